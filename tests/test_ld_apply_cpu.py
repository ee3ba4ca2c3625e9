"""mxa_ld_window_apply / mxa_ld_window_apply_pairwise without a device: the two symbols in every layer that names the C ABI, the reference of the GPU tests
(tests/_ld_apply_ref.py) against a dense long-double product, and the Python argument checks, raised before any library call."""
import ctypes
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

import _ld_apply_ref as ar
import _ld_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mxa_ld_window_apply", "mxa_ld_window_apply_pairwise")
WANT = {"mxa_ld_window_apply": "plink snps indiv last term X ldx n Y ldy is_plink_format allele_freq",
        "mxa_ld_window_apply_pairwise": "plink snps indiv last term X ldx n Y ldy"}


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _header_prototype(sym):
    """[(type, name)] of the header's declaration"""
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
        assert [n for _, n in proto] == WANT[sym].split(), sym
        types = dict((n, t) for t, n in proto)
        assert types["X"] == "const double *" and types["Y"] == "double *" and types["ldx"] == types["ldy"] == "long" and types["n"] == "int", sym
        assert any(fnmatch.fnmatchcase(sym, p) for p in patterns) and sym in exported, sym       # global in the version script, and in the dynamic symbol table
        fn = getattr(L, sym)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None and len(fn.argtypes) == len(proto), sym
        for (t, name), at in zip(proto, fn.argtypes):
            assert at is (ctypes.c_void_p if "*" in t else scalar[t]), (sym, name, t, at)
        assert re.search(r"bind\(C,\s*name='%s'\)" % sym, fortran) and re.search(r"\b%s\b" % sym, public), sym
    comment = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mxa_ld_window_apply\(", _read("include", "miraculix_amd.h"), flags=re.S).group(1)
    assert "for every n" in comment and "fixed order" in comment and "filter such SNPs before the call" in comment
    assert mx.crossproduct.LD_APPLY_NC == ar.NC and tuple(mx.crossproduct.LD_APPLY_TERMS) == ar.TERMS


def test_argument_errors_decided_before_a_device_is_selected(mx):
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    snps, indiv = 5, 8
    X, f, last = np.zeros((snps, 2), np.uint8), np.full(snps, 0.25), np.full(snps, snps - 1, np.int32)
    B = np.ones((2, snps))

    def run(entry, term=1, x=B, ldx=snps, n=2, ldy=snps, with_y=True, nind=indiv):
        Y = np.full((3, snps), -7.5)
        args = [p(X), snps, nind, p(last), term, p(x), ldx, n, p(Y) if with_y else None, ldy] + ([1, p(f)] if entry == SYMBOLS[0] else [])
        return getattr(L, entry)(*args), L.mxa_last_error(), bool(np.all(Y == -7.5))

    for entry in SYMBOLS:
        for bad in (dict(n=0), dict(n=-1), dict(ldx=snps - 1), dict(ldy=snps - 1), dict(term=3), dict(term=-1), dict(term=2, nind=2), dict(x=None), dict(with_y=False)):
            assert run(entry, **bad) == (1, 1, True), (entry, bad, mx.lib.last_error())


def test_the_reference_is_the_dense_windowed_product():
    snps = 40
    rng = np.random.default_rng(3)
    A = rng.standard_normal((snps, snps))
    T = A + A.T                                                   # any symmetric matrix serves as the terms
    X = rng.standard_normal((snps, 5))
    for last in (ref.fixed_last(snps, 0), ref.fixed_last(snps, 7), ref.fixed_last(snps, snps - 1), ref.sweep_window(snps, 1),
                 np.minimum(np.maximum.accumulate(rng.integers(0, snps, snps)), snps - 1).clip(np.arange(snps)).astype(np.int32)):
        assert np.all(np.diff(last) >= 0) and np.all(last >= np.arange(snps))
        got, mag, m = ar.apply_ref(T, last, X)
        want = ar.dense_apply_longdouble(T, last, X)
        first = ref.first_of(last)
        assert np.array_equal(m, last - first + 1)
        # fsum of the float64 products against the long-double product: the products' roundings (2^-53 each) and the long-double sum's (2^-64 each)
        assert np.all(np.abs(got - want.astype(np.float64)) <= 2.0 * ar.U * mag + 1e-300)
        k = 11
        inside = np.arange(snps)[(first <= k) & (k <= last)]
        e = np.zeros((snps, 1))
        e[k] = 1.0
        col = ar.apply_ref(T, last, e)[0][:, 0]
        assert np.array_equal(col[inside], T[inside, k]) and np.all(np.delete(col, inside) == 0.0)
    # the terms in the kernels' operation order
    R = np.array([[1.0, 0.3], [0.3, 1.0]])
    assert ar.terms(R, 10, 0) is R and np.array_equal(ar.terms(R, 10, 1), R * R)
    assert np.array_equal(ar.terms(R, 10, 2), R * R - (1.0 - R * R) * (1.0 / 8.0))
    assert np.array_equal(ar.terms_pw(R, np.full((2, 2), 9.0), 2), R * R - (1.0 - R * R) / 7.0)


def test_python_argument_checks_raise_before_any_library_call(mx, monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(mx.lib, "check_library_handle", no_library)
    snps, indiv = 5, 8
    X, f, last = np.zeros((snps, 2), np.uint8), np.full(snps, 0.25), np.full(snps, snps - 1, np.int32)
    B = np.ones((snps, 3))
    apply_, part = mx.crossproduct.ld_window_apply, mx.crossproduct.ld_scores_partitioned
    for pairwise in (False, True):
        kw = dict(pairwise=pairwise, allele_freq=None if pairwise else f)
        with pytest.raises(ValueError, match="term needs to be"):
            apply_(X, snps, indiv, B, window=2, term="r3", **kw)
        for shape in ((snps + 1, 3), (snps - 1,), (snps, 3, 1), (snps, 0)):
            with pytest.raises(ValueError, match="X needs to be"):
                apply_(X, snps, indiv, np.ones(shape), window=2, **kw)
            with pytest.raises(ValueError, match="X needs to be"):
                part(X, snps, indiv, np.ones(shape), window=2, **kw)
        for bad in (dict(), dict(last=last, window=2)):
            with pytest.raises(ValueError, match="exactly one of last and window"):
                apply_(X, snps, indiv, B, **kw, **bad)
        with pytest.raises(ValueError, match="Window needs to be in"):
            apply_(X, snps, indiv, B, window=snps, **kw)
        with pytest.raises(ValueError, match="at least 3 individuals"):
            apply_(np.zeros((snps, 1), np.uint8), snps, 2, B, window=2, term="r2_adj", **kw)
        with pytest.raises(ValueError, match="out needs to be"):
            apply_(X, snps, indiv, B, window=2, out=np.zeros((snps, 3)), **kw)
    with pytest.raises(ValueError, match="Allele frequencies"):
        apply_(X, snps, indiv, B, window=2)
