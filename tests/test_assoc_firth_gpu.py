"""mxa_assoc_score_firth on the device, against the two references of tests/_assoc_firth_ref.py (the header's definition in np.longdouble run to
|d beta| <= 2^-45 |beta|, and in float64 with the entry's own stop rule).  Inputs: those of tests/test_assoc_spa_gpu.py (rare_case, the nulls fitted by
mxa_assoc_logistic_null, P = y - r), both penalties.

What is asserted per case and penalty: score, var, z and nobs are bit for bit mxa_assoc_score's on the same operands; every flag equals the float64
reference's (the seeds are such that no |z| lies within 2^-40 z_cutoff of the cutoff and, without the penalty, no support margin within [2^-31, 2^-29] A:
asserted, nothing is excluded); over the fitted cells (flag 1) beta and se (relative), chisq / max(1, chisq) and log pval lie within 16 max(eps, 2^-48) of the
long-double reference, eps = the largest of these four differences between the two references over that case's own fitted cells; the references need at most
20 evaluations.  The cells with the flags 0, 2 and 3 carry exactly U / V, 1 / sqrt(V), z z (from the entry's own score, var and z) and the normal p-value
of mxa_assoc_score_spa, or NaN.

eps seen (x86-64, 80-bit long double) and beside it the device's largest of the four differences on an MI355X, without / with the penalty: 6.9e-15 / 9.7e-15
and 9.8e-15 / 1.2e-14 (67, kh 1), 6.4e-15 / 3.7e-15 and 7.0e-15 / 2.4e-15 (259, n 3, kh 3), 2.1e-14 / 2.2e-14 and 1.8e-14 / 9.6e-15 (259, kh 0), 6.9e-15 / 3.9e-15 and
3.7e-15 / 3.7e-15 (1027, kh 17), 9.7e-15 / 8.5e-15 and 1.5e-14 / 8.0e-15 (1027, n 3, kh 3), 3.1e-14 / 8.3e-15 and 3.5e-14 / 1.0e-14 (4099); 300 marked SNPs: 3.2e-14 /
3.5e-14 and 2.3e-13 / 3.6e-13.  The bound is 16 max(eps, 2^-48) = 5.7e-14 at the least.

Shapes: indiv in {67, 259, 1027, 4099} (never a multiple of 4 or 256; 4099: rows of 1025 bytes that start off 16-byte boundaries, 17 individuals per thread
of the solve), snps in {24, 33, 130, 300}, n in {1, 3}, kh in {0, 1, 3, 17}, z_cutoff in {1, 2}."""
import functools
import itertools
import math

import numpy as np
import pytest

import _assoc_firth_ref as fr
import _assoc_spa_ref as sp
import _operands as op

pytestmark = pytest.mark.gpu

SEED = 3
SENTINEL = -7.5
TOL, MAX_ITER = 2.0 ** -30, 50
#        indiv snps n kh z_cutoff
CASES = [(67, 33, 1, 1, 1.0), (259, 130, 3, 3, 2.0), (259, 33, 1, 0, 1.0), (1027, 130, 1, 17, 2.0), (1027, 33, 3, 3, 1.0), (4099, 24, 1, 3, 1.0)]
ROUNDS_CASE = (67, 300, 3, 1)           # 300 marked SNPs: the items cross the 256-SNP rounds of k_assoc_spa_list
DOUBLES = ("score", "var", "z", "beta", "se", "chisq", "pval")
FIT = ("beta", "se", "chisq", "pval")


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(indiv, snps, n, kh):
    """(codes, packed rows, Y, W, P, R, Wt, H): computed once, shared, read-only"""
    import miraculix_amd as m
    return _frozen(*sp.null_operands(m, indiv, snps, n, kh, SEED))


@functools.lru_cache(maxsize=None)
def reference(indiv, snps, n, kh, z_cutoff, penalty):
    codes, _, _, _, P, R, Wt, H = case(indiv, snps, n, kh)
    return fr.both_references(codes, P, R, Wt, H, z_cutoff, penalty, 5)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")


def _columns(M, ld, device):
    rows, cols = M.shape
    buf = np.full((max(cols, 1), ld), np.nan)
    buf[:cols, :rows] = M.T
    return _dev(buf) if device else buf


def run(mx, plink, P, R, Wt, H, z_cutoff=2.0, penalty=1, tol=TOL, max_iter=MAX_ITER, dev=False, ldo=None, want_flag=True, want_nobs=True, want=(True,) * 7):
    """one call through the C ABI, every operand and result on the host or on the device; returns a dict of (snps, n) arrays (None where not asked for) after
    checking that nothing beyond row snps - 1 of a column or beyond column n - 1 was written.  want: score, var, z, beta, se, chisq, pval"""
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    indiv, n = R.shape
    snps = plink.shape[0]
    kh = H.shape[1] // n
    ldo = ldo or snps
    ld = indiv + 1
    new = lambda fill, dt=np.float64: (_dev(np.full((n + 1, ldo), fill, dt)) if dev else np.full((n + 1, ldo), fill, dt))          # noqa: E731
    res = [new(SENTINEL) if w else None for w in want]
    flag = new(-3, np.int32) if want_flag else None
    nobs = (_dev(np.full(snps + 1, -3, np.int32)) if dev else np.full(snps + 1, -3, np.int32)) if want_nobs else None
    X, pb, rb, wb, hb = _dev(plink) if dev else np.ascontiguousarray(plink), *(_columns(M, ld, dev) for M in (P, R, Wt, H))          # (alive until the call is over)
    rc = L.mxa_assoc_score_firth(p(X), snps, indiv, p(pb), ld, p(rb), ld, p(wb), ld, p(hb) if kh else None, ld, n, kh, float(z_cutoff), int(penalty), float(tol),
                                 int(max_iter), *(p(r) for r in res), ldo, p(flag), p(nobs))
    assert rc == 0, mx.lib.last_error()
    out = {}
    for name, r, fill in zip(DOUBLES + ("flag",), res + [flag], (SENTINEL,) * 7 + (-3,)):
        if r is None:
            out[name] = None
            continue
        r = op.readback(r)
        assert np.all(r[n] == fill) and np.all(r[:, snps:] == fill), name
        out[name] = np.ascontiguousarray(r[:n, :snps].T)
    if nobs is not None:
        nobs = op.readback(nobs)
        assert nobs[snps] == -3
        out["nobs"] = nobs[:snps]
    return out


def run_score(mx, plink, R, Wt, H):
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    indiv, n = R.shape
    snps = plink.shape[0]
    kh = H.shape[1] // n
    res = [np.zeros((n, snps)) for _ in range(3)]
    nobs = np.zeros(snps, np.int32)
    X, rb, wb, hb = np.ascontiguousarray(plink), *(_columns(M, indiv, False) for M in (R, Wt, H))
    rc = L.mxa_assoc_score(p(X), snps, indiv, p(rb), indiv, p(wb), indiv, p(hb) if kh else None, indiv, n, kh, p(res[0]), p(res[1]), p(res[2]), snps, p(nobs))
    assert rc == 0, mx.lib.last_error()
    return [r.T for r in res], nobs


def normal_p_of_the_library(mx, plink, P, R, Wt, H):
    """the normal p-value of every cell as mxa_assoc_score_spa writes it with nothing corrected"""
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    indiv, n = R.shape
    snps = plink.shape[0]
    kh = H.shape[1] // n
    z, pv = np.zeros((n, snps)), np.zeros((n, snps))
    X, pb, rb, wb, hb = np.ascontiguousarray(plink), *(_columns(M, indiv, False) for M in (P, R, Wt, H))
    rc = L.mxa_assoc_score_spa(p(X), snps, indiv, p(pb), indiv, p(rb), indiv, p(wb), indiv, p(hb) if kh else None, indiv, n, kh, math.inf, TOL, MAX_ITER, None, None,
                               p(z), p(pv), snps, None, None)
    assert rc == 0, mx.lib.last_error()
    return pv.T


def same(a, b):
    """every array of two results bit for bit"""
    return all((a[k] is None and b[k] is None) or np.array_equal(op.bits(a[k]), op.bits(b[k])) for k in a)


def check_unfitted_cells(mx, got, operands):
    """the cells with the flags 0 and 2 carry exactly the one-step values of the entry's own U, V and z, those with the flag 3 NaN"""
    plink, P, R, Wt, H = operands
    flag, U, V, z = got["flag"], got["score"], got["var"], got["z"]
    one, nan = (flag == 0) | (flag == 2), flag == 3
    assert np.array_equal(nan, ~np.isfinite(z))
    normal = normal_p_of_the_library(mx, plink, P, R, Wt, H)
    with np.errstate(all="ignore"):
        want = {"beta": U / V, "se": 1.0 / np.sqrt(V), "chisq": z * z, "pval": normal}
    for k in FIT:
        assert np.array_equal(op.bits(got[k][one]), op.bits(want[k][one])), k
        assert np.all(np.isnan(got[k][nan])), k
    ok = one & (normal > 1e-200)
    by_hand = np.array([math.erfc(abs(v) / math.sqrt(2.0)) for v in z[ok]])
    assert np.all(np.abs(np.log(got["pval"][ok]) - np.log(by_hand)) <= 16 * 2.0 ** -48)


def check_against(got, rld, flags, eps, what):
    assert np.array_equal(got["flag"], flags), np.argwhere(got["flag"] != flags)[:5]
    err = fr.errors(got, rld, flags == 1)
    bound = 16 * max(eps, 2.0 ** -48)
    print(f"{what}: flags {np.bincount(flags.ravel(), minlength=4)}, eps {eps:.3g}, device " + ", ".join(f"{k} {v:.3g}" for k, v in err.items()) +
          f", bound {bound:.3g}, evaluations <= {rld['evals'].max()}")
    assert max(err.values()) <= bound, err


@pytest.mark.parametrize("penalty", [0, 1])
@pytest.mark.parametrize("indiv, snps, n, kh, z_cutoff", CASES)
def test_flags_and_fits_against_the_references(mx, indiv, snps, n, kh, z_cutoff, penalty):
    codes, plink, Y, W, P, R, Wt, H = case(indiv, snps, n, kh)
    rld, flags, eps = reference(indiv, snps, n, kh, z_cutoff, penalty)
    assert 0.02 < Y.mean() < 0.07 and np.any(codes < 0) and indiv % 4 and indiv % 256
    got = run(mx, plink, P, R, Wt, H, z_cutoff, penalty)
    (score, var, z), nobs = run_score(mx, plink, R, Wt, H)
    for name, want in (("score", score), ("var", var), ("z", z), ("nobs", nobs)):
        assert np.array_equal(op.bits(got[name]), op.bits(want)), name
    check_against(got, rld, flags, eps, f"indiv {indiv} snps {snps} n {n} kh {kh} z_cutoff {z_cutoff} penalty {penalty}")
    check_unfitted_cells(mx, got, (plink, P, R, Wt, H))
    # the same call with everything on the device: the same bits
    assert same(got, run(mx, plink, P, R, Wt, H, z_cutoff, penalty, dev=True))


@functools.lru_cache(maxsize=None)
def edge_case():
    """indiv 67, n = 1, kh = 0 (g = x): SNP 0 entirely missing (N = 0), SNP 1 monomorphic (no minor allele: U = V = 0 exactly), SNP 2 carried by two cases
    alone without a missing call (U = G+ - c0: the edge of the support), then ordinary rows"""
    snps = 12
    codes, plink, Y, W, P, R, Wt, H = case(67, 33, 1, 0)
    codes = codes[:snps].copy()
    codes[0] = -1
    codes[1] = 0
    codes[2] = 0
    codes[2, np.flatnonzero(Y[:, 0] > 0)[:2]] = (1, 2)
    return _frozen(codes, sp.pack(codes)) + (P, R, Wt, H)


@pytest.mark.parametrize("penalty", [0, 1])
def test_edges_all_missing_monomorphic_and_the_edge_of_the_support(mx, penalty):
    codes, plink, P, R, Wt, H = edge_case()
    rld, flags, eps = fr.both_references(codes, P, R, Wt, H, 1.0, penalty, 1)
    assert list(flags[:3, 0]) == [3, 3, 1 if penalty else 2] and set(flags[3:, 0]) <= {0, 1}
    for dev in (False, True):
        got = run(mx, plink, P, R, Wt, H, 1.0, penalty, dev=dev)
        check_against(got, rld, flags, eps, f"edges, penalty {penalty}, device pointers {dev}")
        check_unfitted_cells(mx, got, (plink, P, R, Wt, H))
        assert abs(got["z"][2, 0]) > 2
        if penalty:                            # the maximum-likelihood estimate does not exist; the penalised one is finite and on the carriers' side
            assert np.isfinite(got["beta"][2, 0]) and got["beta"][2, 0] > 0 and got["score"][2, 0] > 0 and np.isfinite(got["se"][2, 0])


def test_an_infinite_cutoff_fits_nothing(mx):
    indiv, snps, n, kh, z_cutoff = CASES[1]
    codes, plink, Y, W, P, R, Wt, H = case(indiv, snps, n, kh)
    for penalty in (0, 1):
        got = run(mx, plink, P, R, Wt, H, math.inf, penalty)
        assert np.all(got["flag"] == 0) and np.all(np.isfinite(got["z"]))
        check_unfitted_cells(mx, got, (plink, P, R, Wt, H))


@functools.lru_cache(maxsize=None)
def short_reference(max_iter, tol, penalty):
    """the float64 reference's flags of CASES[1] under a cap on the evaluations; no item may sit at the stop rule (the flags at 0.99 tol and 1.01 tol are the
    same)"""
    indiv, snps, n, kh, z_cutoff = CASES[1]
    codes, _, _, _, P, R, Wt, H = case(indiv, snps, n, kh)
    flags = [fr.firth_reference(codes, P, R, Wt, H, z_cutoff, penalty, t, max_iter)["flag"] for t in (tol, 0.99 * tol, 1.01 * tol)]
    assert np.array_equal(flags[0], flags[1]) and np.array_equal(flags[0], flags[2])
    return flags[0]


@pytest.mark.parametrize("penalty", [0, 1])
def test_a_cap_on_the_evaluations_fails_some_items_and_solves_others_in_one_batch(mx, penalty):
    indiv, snps, n, kh, z_cutoff = CASES[1]
    codes, plink, Y, W, P, R, Wt, H = case(indiv, snps, n, kh)
    _, full, _ = reference(indiv, snps, n, kh, z_cutoff, penalty)
    one = run(mx, plink, P, R, Wt, H, z_cutoff, penalty, max_iter=1)       # one evaluation solves nothing
    assert np.array_equal(one["flag"], np.where(full == 1, 2, full)) and np.array_equal(one["flag"], short_reference(1, TOL, penalty))
    check_unfitted_cells(mx, one, (plink, P, R, Wt, H))
    loose = 2.0 ** -4                                                      # three evaluations at a loose tolerance: both kinds
    flags = short_reference(3, loose, penalty)
    assert (flags == 1).sum() >= 3 and (flags == 2).sum() >= 3, np.bincount(flags.ravel())
    for dev in (False, True):
        got = run(mx, plink, P, R, Wt, H, z_cutoff, penalty, tol=loose, max_iter=3, dev=dev)
        assert np.array_equal(got["flag"], flags)
        check_unfitted_cells(mx, got, (plink, P, R, Wt, H))


@functools.lru_cache(maxsize=None)
def rounds_reference(penalty):
    """ROUNDS_CASE with the cutoff just below the smallest of the SNPs' largest |z|: every SNP is marked, not every trait"""
    codes, _, _, _, P, R, Wt, H = case(*ROUNDS_CASE)
    z = np.abs(fr.firth_reference(codes, P, R, Wt, H, math.inf)["z"])
    assert np.all(np.isfinite(z))
    z_cutoff = float(0.999 * z.max(axis=1).min())
    return (z_cutoff,) + fr.both_references(codes, P, R, Wt, H, z_cutoff, penalty, 300)


@pytest.mark.parametrize("penalty", [0, 1])
def test_items_across_the_rounds_of_the_list(mx, monkeypatch, penalty):
    codes, plink, Y, W, P, R, Wt, H = case(*ROUNDS_CASE)
    z_cutoff, rld, flags, eps = rounds_reference(penalty)
    marked = flags != 0
    assert np.all(marked.any(axis=1)) and not np.all(marked) and plink.shape[0] == 300
    got = run(mx, plink, P, R, Wt, H, z_cutoff, penalty)
    check_against(got, rld, flags, eps, f"300 marked SNPs, penalty {penalty}")
    check_unfitted_cells(mx, got, (plink, P, R, Wt, H))
    monkeypatch.setenv("MXA_ASSOC_SPA_ITEMS", "4")
    assert same(got, run(mx, plink, P, R, Wt, H, z_cutoff, penalty, dev=True))


def test_dirty_padding_and_a_larger_ldo(mx):
    indiv, snps, n, kh, z_cutoff = CASES[1]
    codes, plink, Y, W, P, R, Wt, H = case(indiv, snps, n, kh)
    assert op.padding_fields(indiv) > 0
    plain = run(mx, plink, P, R, Wt, H, z_cutoff)
    for code in op.CODES:
        assert same(plain, run(mx, op.dirty(plink, indiv, code), P, R, Wt, H, z_cutoff, dev=code in (1, 3)))
    for dev in (False, True):                  # (run checks the sentinels behind row snps - 1 of every column and in the column behind the last)
        assert same(plain, run(mx, plink, P, R, Wt, H, z_cutoff, dev=dev, ldo=snps + 5))


def test_every_combination_of_optional_outputs(mx):
    indiv, snps, n, kh, z_cutoff = CASES[0]
    codes, plink, Y, W, P, R, Wt, H = case(indiv, snps, n, kh)
    plain = run(mx, plink, P, R, Wt, H, z_cutoff)
    count = 0
    for scan in itertools.product((False, True), repeat=3):
        if not any(scan):
            continue                           # (score, var and zstat all NULL is an argument error: tests/test_assoc_firth_cpu.py)
        for se, chisq, pval, want_flag, want_nobs in itertools.product((False, True), repeat=5):
            want = scan + (True, se, chisq, pval)
            part = run(mx, plink, P, R, Wt, H, z_cutoff, dev=count % 2 == 1, want_flag=want_flag, want_nobs=want_nobs, want=want)
            for key, w in zip(DOUBLES + ("flag",), want + (want_flag,)):
                assert (part[key] is None) == (not w) and (not w or np.array_equal(op.bits(part[key]), op.bits(plain[key]))), (key, want)
            assert ("nobs" in part) == want_nobs and (not want_nobs or np.array_equal(part["nobs"], plain["nobs"]))
            count += 1
    assert count == 7 * 32


@pytest.mark.parametrize("indiv, snps, n, kh, z_cutoff", [CASES[1], CASES[5]])
def test_chunks_batches_and_runs_give_the_same_bits(mx, monkeypatch, indiv, snps, n, kh, z_cutoff):
    codes, plink, Y, W, P, R, Wt, H = case(indiv, snps, n, kh)
    for penalty in (0, 1):
        first = run(mx, plink, P, R, Wt, H, z_cutoff, penalty)
        assert same(first, run(mx, plink, P, R, Wt, H, z_cutoff, penalty))
        for name, value in (("MXA_ASSOC_CHUNK_ROWS", "7"), ("MXA_ASSOC_SPA_BATCH", "1"), ("MXA_ASSOC_SPA_BATCH", "5"), ("MXA_ASSOC_SPA_ITEMS", "1"),
                            ("MXA_ASSOC_SPA_ITEMS", "4")):
            monkeypatch.setenv(name, value)
            for dev in (False, True):
                assert same(first, run(mx, plink, P, R, Wt, H, z_cutoff, penalty, dev=dev)), (name, value, dev)
            monkeypatch.delenv(name)


def test_mixed_sides_of_the_results_are_refused(mx):
    codes, plink, Y, W, P, R, Wt, H = case(*CASES[0][:4])
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    indiv, snps = CASES[0][:2]
    z, beta, se, fl = np.full((1, snps), SENTINEL), np.full((1, snps), SENTINEL), np.full((1, snps), SENTINEL), _dev(np.full((1, snps), -3, np.int32))
    zd, sed = _dev(z), _dev(se)
    X, pb, rb, wb, hb = np.ascontiguousarray(plink), *(_columns(M, indiv, False) for M in (P, R, Wt, H))
    args = (p(X), snps, indiv, p(pb), indiv, p(rb), indiv, p(wb), indiv, p(hb), indiv, 1, 1, 2.0, 1, TOL, MAX_ITER)
    assert L.mxa_assoc_score_firth(*args, None, None, p(z), p(beta), None, None, None, snps, p(fl), None) == 1 and L.mxa_last_error() == 1
    assert L.mxa_assoc_score_firth(*args, None, None, p(zd), p(beta), None, None, None, snps, None, None) == 1 and L.mxa_last_error() == 1
    assert L.mxa_assoc_score_firth(*args, None, None, p(z), p(beta), p(sed), None, None, snps, None, None) == 1 and L.mxa_last_error() == 1
    assert "mxa_assoc_score_firth" in mx.lib.last_error()[1]
    assert np.all(z == SENTINEL) and np.all(beta == SENTINEL) and np.all(op.readback(fl) == -3) and np.all(op.readback(sed) == SENTINEL)
    assert np.all(op.readback(zd) == SENTINEL)


def test_the_python_entries_end_to_end(mx):
    import torch
    indiv, snps, n, kh, z_cutoff = CASES[4]
    codes, plink, Y, W, P, R, Wt, H = case(indiv, snps, n, kh)
    rld, flags, eps = reference(indiv, snps, n, kh, z_cutoff, 1)
    want = run(mx, plink, P, R, Wt, H, z_cutoff)
    full = mx.assoc_logistic(plink, snps, indiv, Y, covariates=W, firth=True, z_cutoff=z_cutoff)
    assert isinstance(full, mx.assoc.AssocFirthResult) and np.array_equal(full.flag, flags) and full.flag.dtype == np.int32
    assert max(fr.errors(full._asdict(), rld, flags == 1).values()) <= 16 * max(eps, 2.0 ** -48)
    direct = mx.assoc_score_firth(plink, snps, indiv, P, R, Wt, H, z_cutoff=z_cutoff)
    for a, b, key in zip(full, direct, full._fields):
        assert np.array_equal(op.bits(a), op.bits(b)) and np.array_equal(op.bits(a), op.bits(want[key])), key
    mle = mx.assoc_logistic(plink, snps, indiv, Y, covariates=W, firth=True, z_cutoff=z_cutoff, penalty=0)
    assert np.array_equal(mle.flag, reference(indiv, snps, n, kh, z_cutoff, 0)[1]) and not np.array_equal(op.bits(mle.beta), op.bits(full.beta))
    with pytest.raises(ValueError, match="exclude"):
        mx.assoc_logistic(plink, snps, indiv, Y, covariates=W, spa=True, firth=True)
    plain = mx.assoc_logistic(plink, snps, indiv, Y, covariates=W)
    assert isinstance(plain, mx.assoc.AssocScoreResult) and np.array_equal(op.bits(plain.z), op.bits(full.z))
    dev = mx.assoc_score_firth(_dev(plink), snps, indiv, *(torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (P, R, Wt, H)), z_cutoff=z_cutoff)
    assert dev.beta.is_cuda and dev.flag.is_cuda and dev.flag.dtype == torch.int32 and isinstance(dev.nobs, np.ndarray)
    for a, key in zip(dev[:8], dev._fields):
        assert np.array_equal(op.bits(op.readback(a)), op.bits(want[key])), key
    one = mx.assoc_logistic(plink, snps, indiv, Y[:, 0], covariates=W, firth=True, z_cutoff=z_cutoff, max_iter=40)
    assert one.beta.shape == (snps,) and one.flag.shape == (snps,) and np.array_equal(one.flag, flags[:, 0])
    out = {"beta": np.full((snps, n), SENTINEL, order="F"), "var": np.full((snps, n), SENTINEL, order="F"), "se": np.full((snps, n), SENTINEL, order="F")}
    res = mx.assoc_score_firth(plink, snps, indiv, P, R, Wt, H, z_cutoff=z_cutoff, out=out)
    assert res.beta is out["beta"] and res.var is out["var"] and res.se is out["se"] and res.z is None and res.score is None and res.pval is None
    for key in out:
        assert np.array_equal(op.bits(out[key]), op.bits(want[key])), key
