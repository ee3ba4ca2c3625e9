"""mxa_assoc_set and mxa_assoc_skat_pvalue without a device: the symbols in every layer, the argument errors of mxa_assoc_set (decided before a device is
selected, outputs untouched), mxa_assoc_skat_pvalue against mpmath, and the reference of the GPU tests against itself.

The p-value bound.  The log-scale argument a log x - x - lgamma(a) is at most 745 in magnitude where the result is a double and is computed in long double:
745 2^-63 ~ 2^-53 relative.  The rest of 2^-40 is margin for the series and the continued fraction.  The issue's grid is asserted at EVERY point with a positive
x, whatever the size of the reference value (the smallest, at l = 0.05 and x = 1400, is a subnormal double of some 4e-309: its spacing is still 2^-49 of it).
Measured maximum over the grid: see DESIGN.md 3.6i."""
import ctypes
import fnmatch
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _assoc_set_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("mxa_assoc_set", "mxa_assoc_skat_pvalue")
LD = sr.LD


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


def test_both_entries_are_in_every_layer_with_the_headers_prototype(mx):
    fortran = _read("miraculix_amd", "bindings", "fortran", "modmiraculix_amd.f90")
    public = " ".join(re.findall(r"^\s*public\s*::(.*)$", fortran, flags=re.M))
    patterns = re.findall(r"([\w*]+)\s*;", re.sub(r"/\*.*?\*/", "", _read("miraculix_amd", "csrc", "exports.map"), flags=re.S).split("local:")[0])
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "miraculix_amd", "lib", "libmiraculix_amd.so")],
                                                                 text=True).splitlines() if ln.strip()}
    assert len(exported) == 80
    scalar = {"int": ctypes.c_int, "long": ctypes.c_long, "double": ctypes.c_double}
    for sym in SYMS:
        proto = _header_prototype(sym)
        assert any(fnmatch.fnmatchcase(sym, p) for p in patterns) and sym in exported
        fn = getattr(mx.lib.check_library_handle(), sym)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(proto)
        for (t, name), at in zip(proto, fn.argtypes):
            assert at is (ctypes.c_void_p if "*" in t else scalar[t]), (name, t, at)
        block = re.search(r"function %s\((.*?)\)\s*&?\s*bind\(C,\s*name='%s'\)" % (sym, sym), fortran, flags=re.S)
        assert block and re.search(r"\b%s\b" % sym, public)
        assert len(re.sub(r"[&\s]", "", block.group(1)).split(",")) == len(proto)
    assert [n for _, n in _header_prototype("mxa_assoc_set")] == ["plink", "snps", "indiv", "R", "ldr", "Wt", "ldw", "H", "ldh", "n", "kh", "nsets", "set_ptr", "set_idx",
                                                                  "set_wt", "score", "var", "zstat", "ldo", "nobs", "stat", "lds", "phi"]
    header = _read("include", "miraculix_amd.h")
    comment = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mxa_assoc_set\(", header, flags=re.S).group(1)
    for phrase in ("no atomics", "MXA_ASSOC_SET_BATCH", "MXA_ASSOC_CHUNK_ROWS", "outputs untouched", "bit for bit", "m_k > 1024", "do not\n * depend on which other sets"):
        assert phrase in comment, phrase
    assert mx.assoc_set is mx.assoc.assoc_set and mx.assoc_skat_pvalue is mx.assoc.assoc_skat_pvalue and mx.assoc_logistic_sets is mx.assoc.assoc_logistic_sets
    assert mx.assoc.AssocSetResult._fields == ("burden", "burden_var", "skat", "c1", "c2", "c4", "burden_p", "skat_p", "skat_df", "phi")
    host = _read("miraculix_amd", "csrc", "mxa_assoc_set_host.h")
    assert "assoc_set_args" in host and "skat_pvalue_host" in host and "hip/" not in host


def test_argument_errors_are_decided_before_a_device_is_selected(mx):
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    snps, indiv, n, kh, nsets = 5, 12, 2, 3, 3
    X = np.zeros((snps, 3), np.uint8)
    R, Wt, H = np.ones((n, indiv)), np.ones((n, indiv)), np.ones((n * kh, indiv))
    PTR, IDX, WTS = np.array([0, 2, 2, 5], np.int64), np.array([4, 0, 1, 1, 3], np.int32), np.ones(5)

    def run(plink=X, snps_=snps, indiv_=indiv, r=R, ldr=indiv, wt=Wt, ldw=indiv, h=H, ldh=indiv, n_=n, kh_=kh, nsets_=nsets, ptr=PTR, idx=IDX, wts=WTS, outs=(1, 1, 1),
            ldo=snps, stat=True, lds=nsets, phi=True):
        res = [np.full((n + 1, snps + 2), -7.5) for _ in range(3)]
        st, ph, nobs = np.full((6 * n + 1, nsets + 2), -7.5), np.full(n * 13 + 3, -7.5), np.full(snps, -3, np.int32)
        rc = L.mxa_assoc_set(p(plink), snps_, indiv_, p(r), ldr, p(wt), ldw, p(h), ldh, n_, kh_, nsets_, p(ptr), p(idx), p(wts),
                             *[p(a) if o else None for a, o in zip(res, outs)], ldo, p(nobs), p(st) if stat else None, lds, p(ph) if phi else None)
        return rc, L.mxa_last_error(), all(bool(np.all(a == -7.5)) for a in res + [st, ph]) and bool(np.all(nobs == -3))

    big = 47453133
    score_errors = (dict(plink=None), dict(r=None), dict(wt=None), dict(snps_=0), dict(indiv_=0), dict(n_=0), dict(n_=-1), dict(kh_=-1), dict(h=None), dict(ldr=indiv - 1),
                    dict(ldw=indiv - 1), dict(ldh=indiv - 1), dict(ldo=snps - 1), dict(indiv_=big, ldr=big, ldw=big, ldh=big), dict(n_=13108, kh_=3), dict(n_=1, kh_=65534))
    too_long = np.concatenate([[0], np.full(3, 1025)]).astype(np.int64)
    own_errors = (dict(nsets_=0), dict(nsets_=-2), dict(ptr=None), dict(idx=None), dict(stat=False), dict(ptr=np.array([1, 2, 2, 5], np.int64)),
                  dict(ptr=np.array([0, 3, 2, 5], np.int64)), dict(idx=np.array([4, 0, 1, 1, 5], np.int32)), dict(idx=np.array([4, -1, 1, 1, 3], np.int32)),
                  dict(ptr=too_long, idx=np.zeros(1025, np.int32), wts=None), dict(lds=nsets - 1))
    for bad in score_errors + own_errors:
        assert run(**bad) == (1, 1, True), (bad, mx.lib.last_error())
        assert "mxa_assoc_set" in mx.lib.last_error()[1]
    for kw, words in ((dict(idx=np.array([4, 0, 1, 1, 5], np.int32)), "entry 2 of set 2"), (dict(idx=np.array([4, -1, 1, 1, 3], np.int32)), "entry 1 of set 0"),
                      (dict(ptr=np.array([0, 3, 2, 5], np.int64)), "decreases at set 1"), (dict(ptr=too_long, idx=np.zeros(1025, np.int32), wts=None), "1025 entries"),
                      (dict(lds=2), "lds"), (dict(nsets_=0), "nsets"), (dict(ptr=np.array([1, 2, 2, 5], np.int64)), "set_ptr[0]")):
        run(**kw)
        assert words in mx.lib.last_error()[1], (words, mx.lib.last_error())
    # valid calls pass the argument checks: they fail loudly for want of a device, or run where there is one -- never code 1, never a crash.  "All three scan
    # results NULL" is no error here.
    for kw in (dict(outs=(0, 0, 0)), dict(wts=None), dict(phi=False), dict(h=None, kh_=0), dict(ptr=np.array([0, 0, 0, 0], np.int64), wts=None)):
        rc, err, _ = run(**kw)
        assert (rc, err) == (0, 0) or (rc == 1 and err != 1), (kw, mx.lib.last_error())


def test_the_stand_alone_sanitizer_program_passes(tmp_path):
    """tools/assoc_set_host_check.cpp, compiled here for the CPU with the sanitizers' runtimes linked statically, so that the program is self-contained; run as a
    plain child process in the inherited environment"""
    exe = str(tmp_path / "assoc_set_host_check")
    build = subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                            os.path.join(ROOT, "tools", "assoc_set_host_check.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("PASS"), run.stdout[-3000:]


GRID_L = (0.05, 0.3, 1.0, 1.937, 7.5, 40.0, 512.0)


def _grid():
    for l in GRID_L:
        for x in (1e-8, 0.1, l - 1, l, l + 1, 50.0, 200.0, 900.0, 1400.0):
            if x > 0:
                yield l, x


def _pvalue_of(mx, l, x):
    """the moments of this l and x: c2 = c4 = l (l = c2^2 / c4, sqrt(l / c2) = 1), c1 = 0, Q = x - l rounded to a double; the x the entry then sees is the exact
    sum Q + l (in long double: off by at most 2^-64 l, which moves no p-value of the grid by more than 2^-46 of itself), and it is what the reference gets"""
    import mpmath
    q = x - l
    pv, df = mx.assoc_skat_pvalue([q], [0.0], [l], [l])
    with mpmath.workdps(50):
        return float(pv[0]), float(df[0]), mpmath.mpf(q) + mpmath.mpf(l)


def test_skat_pvalue_against_mpmath_on_the_grid(mx):
    import mpmath
    worst = 0.0
    for l, x in _grid():
        got, df, x_eff = _pvalue_of(mx, l, x)
        ref = sr.upper_gamma(l, x_eff)
        err = float(abs(mpmath.mpf(got) - ref) / ref)
        worst = max(worst, err)
        print(f"l {l:8.3f} x {float(x_eff):10.4g} ref {mpmath.nstr(ref, 8):>14s} rel.err {err:.3e}")
        assert df == l
        assert err <= 2.0 ** -40, (l, x, got, ref, err)
    print("largest relative error", worst)


def test_skat_pvalue_edges(mx):
    pv, df = mx.assoc_skat_pvalue([1.0, 0.5, -3.0], [3.0, 2.5, 0.0], [2.0, 2.0, 1.0], [2.0, 2.0, 1.0])     # x = 0, x < 0, x < 0
    assert np.array_equal(pv, [1.0, 1.0, 1.0]) and np.array_equal(df, [2.0, 2.0, 1.0])
    nan, inf = math.nan, math.inf
    bad = [(nan, 1, 1, 1), (1, nan, 1, 1), (1, 1, nan, 1), (1, 1, 1, nan), (inf, 1, 1, 1), (1, -inf, 1, 1), (1, 1, inf, 1), (1, 1, 1, inf), (1, 1, 0.0, 1), (1, 1, -1.0, 1),
           (1, 1, 1, 0.0), (1, 1, 1, -2.0), (1, 1, -0.0, 1)]
    q, c1, c2, c4 = (np.array(col, dtype=np.float64) for col in zip(*bad))
    pv, df = mx.assoc_skat_pvalue(q, c1, c2, c4)
    assert np.all(np.isnan(pv)) and np.all(np.isnan(df))
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    one = np.ones(1)
    out = np.full(1, -7.5)
    assert L.mxa_assoc_skat_pvalue(1, p(one), p(one), p(one), p(one), p(out), None) == 0 and 0 < out[0] < 1          # df is optional
    assert L.mxa_assoc_skat_pvalue(0, None, None, None, None, None, None) == 0
    out[:] = -7.5
    assert L.mxa_assoc_skat_pvalue(-1, p(one), p(one), p(one), p(one), p(out), None) == 1 and L.mxa_last_error() == 1 and out[0] == -7.5
    assert L.mxa_assoc_skat_pvalue(1, p(one), None, p(one), p(one), p(out), None) == 1 and L.mxa_last_error() == 1 and out[0] == -7.5
    # one chi-square: Q = z^2 with A = (1): the p-value is erfc(|z| / sqrt 2)
    pv, _ = mx.assoc_skat_pvalue([4.0], [1.0], [1.0], [1.0])
    assert abs(pv[0] - math.erfc(2.0 / math.sqrt(2.0))) <= 2.0 ** -50 * pv[0]


@pytest.fixture(scope="module")
def null_case():
    """a fitted logistic null (long double Newton) with two covariates, 5 % missing calls, sets of several shapes with random weights"""
    from _assoc_score_ref import binary_case, newton_ld
    indiv, snps = 259, 30
    codes, Y, W = binary_case(indiv, snps, 2, 2, seed=4)
    C = np.column_stack([np.ones(indiv), W])
    fits = [newton_ld(Y[:, c], C) for c in range(2)]
    R = np.stack([np.asarray(f[1], np.float64) for f in fits], 1)
    Wt = np.stack([np.asarray(f[2], np.float64) for f in fits], 1)
    H = np.concatenate([np.asarray(f[3], np.float64) for f in fits], 1)
    rng = np.random.default_rng(8)
    sets = [np.arange(0, 8), np.array([29, 3, 3, 17, 5]), np.array([11]), np.array([], np.int64), rng.integers(0, snps, 21)]
    weights = [rng.uniform(0.5, 3.0, len(s)) for s in sets]
    return codes, R, Wt, H, sets, weights


def test_the_two_evaluations_of_the_reference_agree(null_case):
    codes, R, Wt, H, sets, weights = null_case
    ld = sr.set_reference(codes, R, Wt, H, sets, weights, LD)
    f64 = sr.set_reference(codes, R, Wt, H, sets, weights, np.float64)
    indiv = codes.shape[1]
    for a, b in zip(ld, f64):
        # float64 sums of `indiv` terms and chains of a few more: (indiv + 16) 2^-53 of the scale, for any order
        assert sr.scaled_error(b["phi"], a["phi"], a["sphi"]) <= (indiv + 16) * 2.0 ** -53
        for t in range(6):
            assert sr.scaled_error(b["stat"][:, t], a["stat"][:, t], a["sstat"][:, t]) <= 4 * (indiv + 16) * 2.0 ** -53, t


def test_the_references_phi_is_positive_semidefinite_and_df_is_at_most_m(null_case):
    codes, R, Wt, H, sets, weights = null_case
    for k, res in enumerate(sr.set_reference(codes, R, Wt, H, sets, weights, LD)):
        m = len(sets[k])
        for c in range(R.shape[1]):
            phi = np.asarray(res["phi"][c], np.float64)
            if m == 0:
                assert np.array_equal(res["stat"][c], np.zeros(6))
                continue
            assert np.array_equal(phi, phi.T)
            ev = np.linalg.eigvalsh(phi)
            assert ev.min() >= -m * 2.0 ** -45 * np.asarray(res["sphi"][c], np.float64).max(), (k, c, ev.min())
            B, vB, Q, c1, c2, c4 = (float(v) for v in res["stat"][c])
            assert c2 * c2 / c4 <= m * (1 + 2.0 ** -40) and vB > 0 and c1 > 0
            lam = np.linalg.eigvalsh(np.asarray(weights[k])[:, None] * phi * np.asarray(weights[k])[None, :])
            for got, want in ((c1, lam.sum()), (c2, (lam ** 2).sum()), (c4, (lam ** 4).sum())):
                assert abs(got - want) <= 1e-9 * want


def test_a_tuple_is_always_the_csr_pair_and_a_list_always_index_arrays(mx):
    """(array([0, 3]), array([5, 7, 9])) could be read either way by its contents: the type decides, and a pair that is no CSR list is refused"""
    csr = mx.assoc._set_csr
    ptr, idx, wt = csr([np.array([0, 3]), np.array([5, 7, 9])], None)
    assert ptr.tolist() == [0, 2, 5] and idx.tolist() == [0, 3, 5, 7, 9] and wt is None
    ptr, idx, wt = csr((np.array([0, 3]), np.array([5, 7, 9])), [1.0, 2.0, 3.0])
    assert ptr.tolist() == [0, 3] and idx.tolist() == [5, 7, 9] and wt.tolist() == [1.0, 2.0, 3.0] and ptr.dtype == np.int64 and idx.dtype == np.int32
    for bad in ((np.array([0, 2]), np.array([5, 7, 9])), (np.array([1, 3]), np.array([5, 7, 9])), (np.array([0, 3, 2]), np.array([5, 7])), (np.array([0, 1]),),
                (np.array([4, 2]), np.array([1]), np.array([3])), np.array([[0, 1]])):
        with pytest.raises(ValueError):
            csr(bad, None)
