"""mxa_assoc_basis / mxa_assoc_linear without a device: the two symbols in every layer that names the C ABI, the argument errors (decided before a device is
selected), the host-only covariate basis, the Python argument checks, and the references of the GPU tests (tests/_assoc_ref.py) checked against themselves."""
import ctypes
import fnmatch
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _assoc_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mxa_assoc_basis", "mxa_assoc_linear")
WANT = {"mxa_assoc_basis": "int indiv, const double * W, long ldw, int q, double * Q, long ldq",
        "mxa_assoc_linear": "const unsigned char * plink, int snps, int indiv, const double * Y, long ldy, int n, const double * Q, long ldq, int k, double * beta, "
                            "double * se, double * tstat, long ldo, int * nobs, int * dof"}


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
    scalar = {"int": ctypes.c_int, "long": ctypes.c_long}
    for sym in SYMBOLS:
        proto = _header_prototype(sym)
        assert ", ".join(f"{t} {n}" for t, n in proto) == WANT[sym], sym
        assert any(fnmatch.fnmatchcase(sym, p) for p in patterns) and sym in exported, sym
        fn = getattr(L, sym)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None and len(fn.argtypes) == len(proto), sym
        for (t, name), at in zip(proto, fn.argtypes):
            assert at is (ctypes.c_void_p if "*" in t else scalar[t]), (sym, name, t, at)
        assert re.search(r"bind\(C,\s*name='%s'\)" % sym, fortran) and re.search(r"\b%s\b" % sym, public), sym
    comment = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mxa_assoc_basis\(", _read("include", "miraculix_amd.h"), flags=re.S).group(1)
    for phrase in ("NOT promised bit-identical between different n", "fma(mu, M_b - T_b, D_b)", "MXA_ASSOC_CHUNK_ROWS", "no atomics", "There is no special case"):
        assert phrase in comment, phrase
    assert mx.assoc_basis is mx.assoc.assoc_basis and mx.assoc_linear is mx.assoc.assoc_linear
    assert "mxa_assoc.hip" in _read("miraculix_amd", "csrc", "Makefile")
    assert "hip/" not in _read("miraculix_amd", "csrc", "mxa_assoc_host.h")          # the host-only part compiles without HIP


def test_linear_argument_errors_decided_before_a_device_is_selected(mx):
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    snps, indiv, n, k = 5, 12, 2, 3
    X = np.zeros((snps, 3), np.uint8)
    Y, Q = np.ones((n, indiv)), np.ones((k, indiv))

    def run(plink=X, snps_=snps, indiv_=indiv, y=Y, ldy=indiv, n_=n, q=Q, ldq=indiv, k_=k, outs=(1, 1, 1), ldo=snps):
        res = [np.full((n + 1, snps + 2), -7.5) for _ in range(3)]
        nobs, dof = np.full(snps, -3, np.int32), ctypes.c_int(-3)
        rc = L.mxa_assoc_linear(p(plink), snps_, indiv_, p(y), ldy, n_, p(q), ldq, k_, *[p(r) if o else None for r, o in zip(res, outs)], ldo, p(nobs),
                                ctypes.byref(dof))
        return rc, L.mxa_last_error(), all(bool(np.all(r == -7.5)) for r in res) and bool(np.all(nobs == -3)) and dof.value == -3

    for bad in (dict(plink=None), dict(y=None), dict(snps_=0), dict(indiv_=0), dict(n_=0), dict(n_=-1), dict(k_=-1), dict(q=None), dict(ldy=indiv - 1),
                dict(ldq=indiv - 1), dict(ldo=snps - 1), dict(indiv_=5, ldy=5, ldq=5), dict(indiv_=47453133, ldy=47453133, ldq=47453133), dict(outs=(0, 0, 0)),
                dict(indiv_=70000, ldy=70000, ldq=70000, n_=65533, k_=3)):
        assert run(**bad) == (1, 1, True), (bad, mx.lib.last_error())
    assert "degrees of freedom" in (run(indiv_=5, ldy=5, ldq=5), mx.lib.last_error()[1])[1]
    # k = 0 takes a NULL Q: the call passes the argument checks and fails for want of a device (or runs where there is one), never with code 1
    rc, code, _ = run(q=None, k_=0)
    assert code != 1, mx.lib.last_error()


def test_basis_argument_errors_leave_q_untouched(mx):
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    indiv, q = 9, 2
    rng = np.random.default_rng(5)
    W = np.asfortranarray(rng.standard_normal((indiv, q)))

    def run(w=W, indiv_=indiv, ldw=indiv, q_=q, with_q=True, ldq=indiv):
        Q = np.full((q + 1, indiv + 1), -7.5)
        rc = L.mxa_assoc_basis(indiv_, p(w), ldw, q_, p(Q) if with_q else None, ldq)
        return rc, L.mxa_last_error(), bool(np.all(Q == -7.5))

    bad_nan, bad_inf = W.copy(order="F"), W.copy(order="F")
    bad_nan[3, 1], bad_inf[0, 0] = np.nan, np.inf
    for bad in (dict(w=None), dict(with_q=False), dict(q_=-1), dict(ldw=indiv - 1), dict(ldq=indiv - 1), dict(indiv_=0, ldw=0, ldq=0), dict(w=bad_nan), dict(w=bad_inf)):
        assert run(**bad) == (1, 1, True), (bad, mx.lib.last_error())
    const = W.copy(order="F")
    const[:, 1] = 4.25
    assert run(w=const) == (1, 1, True) and "column 1" in mx.lib.last_error()[1]
    dup = np.asfortranarray(np.stack([W[:, 0], W[:, 1], 2.0 * W[:, 0] + 3.0], axis=1))
    Q3 = np.full((3, indiv), -7.5)
    assert L.mxa_assoc_basis(indiv, p(dup), indiv, 3, p(Q3), indiv) == 1 and L.mxa_last_error() == 1 and np.all(Q3 == -7.5)
    assert "column 2" in mx.lib.last_error()[1]
    with pytest.raises(RuntimeError, match="column 2"):
        mx.assoc_basis(dup)
    assert run(q_=0) == (0, 0, True)


@pytest.mark.parametrize("indiv, q", [(7, 1), (67, 5), (1027, 16), (4099, 10)])
def test_basis_is_orthonormal_zero_sum_and_spans_the_centred_covariates(mx, indiv, q):
    rng = np.random.default_rng([11, indiv, q])
    W = rng.standard_normal((indiv, q)) * rng.uniform(0.5, 20, q) + rng.uniform(-100, 100, q) + 0.5 * rng.standard_normal((indiv, 1))
    Q = mx.assoc_basis(W)
    assert Q.shape == (indiv, q) and Q.flags.f_contiguous
    tol = 8 * indiv * ar.U
    QL = Q.astype(ar.LD)
    assert np.abs(QL.T @ QL - np.eye(q)).max() <= tol
    assert np.abs(QL.sum(0)).max() <= tol
    Wc = W.astype(ar.LD) - W.astype(ar.LD).mean(0)
    # the spans are equal: each side is reproduced by its projection onto the other (the centred W through Q; Q through a least-squares fit on the centred W)
    assert np.abs(Wc - QL @ (QL.T @ Wc)).max() <= 64 * indiv * ar.U * np.abs(Wc).max()
    coef = np.linalg.lstsq(Wc.astype(np.float64), Q, rcond=None)[0]
    assert np.abs(Wc.astype(np.float64) @ coef - Q).max() <= 1e-9
    # in place order: column j depends on the columns up to j alone
    assert np.array_equal(mx.assoc_basis(W[:, : max(1, q // 2)]), Q[:, : max(1, q // 2)])
    # leading dimensions larger than needed: the rows beyond indiv are neither read nor written
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    Wp, Qp = np.full((q, indiv + 3), np.nan), np.full((q, indiv + 2), -7.5)
    Wp[:, :indiv] = W.T
    assert L.mxa_assoc_basis(indiv, p(Wp), indiv + 3, q, p(Qp), indiv + 2) == 0
    assert np.array_equal(Qp[:, :indiv].T, Q) and np.all(Qp[:, indiv:] == -7.5)


def test_python_argument_checks_raise_before_any_library_call(mx, monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(mx.lib, "check_library_handle", no_library)
    snps, indiv = 5, 12
    X, Y, Q = np.zeros((snps, 3), np.uint8), np.ones((indiv, 2)), np.ones((indiv, 3))
    with pytest.raises(ValueError, match="wrong dimensions"):
        mx.assoc_linear(np.zeros((snps, 4), np.uint8), snps, indiv, Y)
    with pytest.raises(ValueError, match="positive"):
        mx.assoc_linear(X, 0, indiv, Y)
    for shape in ((indiv + 1, 2), (indiv - 1,), (indiv, 2, 1), (indiv, 0)):
        with pytest.raises(ValueError, match="Y needs to be"):
            mx.assoc_linear(X, snps, indiv, np.ones(shape))
    with pytest.raises(ValueError, match="Q needs to be"):
        mx.assoc_linear(X, snps, indiv, Y, Q=np.ones((indiv + 1, 3)))
    with pytest.raises(ValueError, match="at most one of covariates and Q"):
        mx.assoc_linear(X, snps, indiv, Y, covariates=Q, Q=Q)
    with pytest.raises(ValueError, match="covariates need to be"):
        mx.assoc_linear(X, snps, indiv, Y, covariates=np.ones((indiv - 1, 2)))
    with pytest.raises(ValueError, match="degrees of freedom"):
        mx.assoc_linear(X, snps, indiv, Y, Q=np.ones((indiv, indiv - 2)))
    with pytest.raises(ValueError, match="degrees of freedom"):
        mx.assoc_linear(X, snps, indiv, Y, covariates=np.ones((indiv, indiv - 2)))
    with pytest.raises(ValueError, match="at most"):
        mx.assoc_linear(np.zeros((1, 1), np.uint8), 1, 47453133, Y)
    for out in ({}, {"p": np.zeros((snps, 2), order="F")}, {"beta": np.zeros((snps, 2))}, {"se": np.zeros((snps, 3), order="F")},
                {"t": np.zeros((snps, 2), np.float32, order="F")}):
        with pytest.raises(ValueError, match="out"):
            mx.assoc_linear(X, snps, indiv, Y, Q=Q, out=out)
    with pytest.raises(ValueError, match="covariates need to be"):
        mx.assoc_basis(np.ones((2, 3, 4)))
    with pytest.raises(ValueError, match="finite"):
        mx.assoc_basis(np.array([[1.0, np.nan], [2.0, 3.0], [0.0, 1.0]]))


def test_packing_and_the_exact_family_are_what_they_claim():
    codes = np.array([[0, 1, 2, -1, 2], [-1, -1, 0, 0, 1]], np.int8)
    assert np.array_equal(ar.pack(codes), np.array([[0b01111000, 0b11], [0b00000101, 0b10]], np.uint8))
    for indiv, n, k in ((19, 1, 0), (19, 3, 14), (67, 17, 16), (259, 2, 15), (1027, 3, 4)):
        Y, Q = ar.exact_family(indiv, n, k, seed=3)
        assert np.array_equal(Q.T @ Q, np.eye(k)) and np.all(Q.sum(0) == 0) and np.all(Q.T @ Y == 0) and np.all(Y.sum(0) == 0)
        assert np.all(Y == np.round(Y)) and np.abs(Y[: indiv - 3]).max() <= 12 and np.all(Q[indiv - 3:] == 0)
        # every sum the definition names is exact in fp64 in any order: float64 sums in two orders against rational arithmetic
        codes = ar.genotypes(9, indiv, seed=4)
        B = np.concatenate([Y, Q], axis=1)
        N, Sz, Szz, D, M, T = ar.sums(codes, B)
        _, _, _, Dr, Mr, Tr = ar.sums(codes[:, ::-1], B[::-1])
        assert np.array_equal(D, Dr) and np.array_equal(M, Mr) and np.array_equal(T, Tr)
        for s in (0, 3, 8):
            for b in (0, n + k - 1):
                col = [Fraction(float(v)) for v in B[:, b]]
                assert Fraction(float(D[s, b])) == sum(c * int(max(g, 0)) for c, g in zip(col, codes[s]))
                assert Fraction(float(M[s, b])) == sum(c for c, g in zip(col, codes[s]) if g < 0)
        assert N[0] == 0 and N[1] == 1 and N[2] == indiv and codes[4, -1] == -1 and not np.any(codes[5] < 0)
    assert ar.fma(3.0, 1.0 / 3.0, -1.0) == float(Fraction(3.0) * Fraction(1.0 / 3.0) - 1) != 3.0 * (1.0 / 3.0) - 1.0
    assert str(ar.fma(-0.0, 0.0, 0.0)) == "0.0" and str(ar.fma(-0.0, 0.0, -0.0)) == "-0.0" and np.isnan(ar.fma(np.nan, 1.0, 1.0)) and ar.div(1.0, 0.0) == np.inf
    # the chain on the edge rows: N = 0 and a SNP constant on its called individuals give non-finite results, every other SNP finite ones
    Y, Q = ar.exact_family(67, 2, 3, seed=1)
    beta, se, t, nobs = ar.chain_exact(ar.genotypes(12, 67, seed=2), Y, Q)
    assert np.all(np.isnan(beta[0])) and not np.any(np.isfinite(t[[0, 2, 3]])) and np.all(np.isfinite(beta[5:])) and np.all(np.isfinite(se[5:]))
    assert nobs[0] == 0 and nobs[1] == 1 and nobs[2] == 67


def test_the_reference_agrees_with_least_squares_on_the_mean_imputed_design(mx):
    indiv, snps, n, k = 300, 12, 2, 3
    codes, Y, W = ar.real_case(indiv, snps, n, k, seed=7)
    Q = mx.assoc_basis(W)
    (beta, se, t), _, sxx, v0 = ar.bounded(codes, Y, Q)
    assert np.any(codes < 0)
    for s in range(snps):
        x = codes[s].astype(np.float64)
        x[codes[s] < 0] = x[codes[s] >= 0].mean()
        X = np.column_stack([np.ones(indiv), W, x])
        Xs = X / np.linalg.norm(X, axis=0)
        assert np.linalg.cond(Xs) < 100
        coef, res, _, _ = np.linalg.lstsq(Xs, Y, rcond=None)
        b = coef[-1] / np.linalg.norm(X[:, -1])
        assert np.abs(b - beta[s].astype(np.float64)).max() <= 1e-9 * np.abs(b).max()
        resid = Y - Xs @ coef
        sigma2 = (resid ** 2).sum(0) / (indiv - k - 2)
        cov = np.linalg.inv(Xs.T @ Xs)[-1, -1] / np.linalg.norm(X[:, -1]) ** 2
        assert np.abs(np.sqrt(sigma2 * cov) - se[s].astype(np.float64)).max() <= 1e-8 * np.sqrt(sigma2 * cov).max()


@pytest.mark.parametrize("indiv", [67, 1027, 4099])
@pytest.mark.parametrize("n, k", [(1, 3), (8, 10)])
def test_a_float64_restatement_in_reversed_order_meets_the_bound_of_the_gpu_test(mx, indiv, n, k):
    """the bound of tests/test_assoc_gpu.py is one a correct implementation can meet: plain float64 numpy, the individuals summed in reversed order"""
    codes, Y, W = ar.real_case(indiv, 513, n, k, seed=21)
    Q = mx.assoc_basis(W)
    ref, bound, sxx, v0 = ar.bounded(codes, Y, Q)
    keep = sxx >= 1e-6 * v0
    assert np.all(keep)
    got = ar.restate_float64(codes, Y, Q, reverse=True)
    for name, g, r, b in zip(("beta", "se", "t"), got, ref, bound):
        ok, ratio = ar.within_bound(g, r, b, keep)
        print(f"indiv {indiv} n {n} k {k} {name}: max |err| / bound = {ratio:.3g}")
        assert ok, (name, ratio)
