"""mxa_assoc_score_spa on the device, against the two references of tests/_assoc_spa_ref.py (the header's definition in np.longdouble run to |dt| <= 2^-45 |t|,
and in float64 with the entry's own stop rule).  Inputs: rare_case (binary_case at 3-5 % cases, every fourth SNP at MAF 0.01, 5 % missing calls), the nulls
fitted by mxa_assoc_logistic_null, P = y - r.

What is asserted per case: score, var, z and nobs are bit for bit mxa_assoc_score's on the same operands; the flags equal the references' everywhere (the
seeds are such that no item lies within 2^-40 z_cutoff of the cutoff and no support margin within [2^-31, 2^-29] A: asserted, nothing is excluded); every
finite p-value above 1e-200 meets |log pval - log p_LD| <= 16 max(eps, 2^-48), eps = the largest |log p_64 - log p_LD| between the two references over that
case's own entries; the reference needs at most 12 evaluations.  The factor 16 covers the device's summation order and its few-ulp exp / log / erfc.

eps seen (x86-64, 80-bit long double), and beside it the device's largest |log pval - log p_LD| on an MI355X: 1.9e-15 / 3.0e-15 (67, kh 1), 6.0e-15 / 2.8e-15
(259, n 3, kh 3), 4.3e-15 / 4.0e-15 (259, kh 0), 5.6e-15 / 3.9e-15 (1027, kh 17), 2.5e-15 / 4.0e-15 (1027, n 3, kh 3), 1.4e-14 / 3.3e-15 (4099), 6.1e-14 / 1.9e-14
(16387).  The bound is 16 max(eps, 2^-48) = 5.7e-14 at the least.

Shapes: indiv in {67, 259, 1027, 4099, 16387} (4099: 24 SNPs, n = 1, kh = 3, rows of 1025 bytes that start off 16-byte boundaries; 16387: more than one
64-individual word per thread of the scan, 65 individuals per thread of the solve), snps in {33, 130}, n in {1, 3}, kh in {0, 1, 3, 17}, z_cutoff in {1, 2}."""
import functools
import math

import numpy as np
import pytest

import _assoc_spa_ref as sp
import _operands as op

pytestmark = pytest.mark.gpu

SEED = 3
SENTINEL = -7.5
TOL, MAX_ITER = 2.0 ** -30, 50
#        indiv snps n kh z_cutoff
CASES = [(67, 33, 1, 1, 1.0), (259, 130, 3, 3, 2.0), (259, 33, 1, 0, 1.0), (1027, 130, 1, 17, 2.0), (1027, 33, 3, 3, 1.0), (4099, 24, 1, 3, 1.0),
         (16387, 24, 1, 3, 1.0)]


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


def both_references(codes, P, R, Wt, H, z_cutoff, least):
    """(p_LD, flags, eps) after the checks on the inputs that the module's docstring names; least: the corrected items the case must have"""
    p64, f64, z64, e64, _ = sp.spa_reference(codes, P, R, Wt, H, z_cutoff, TOL, MAX_ITER, np.float64)
    pld, fld, _, eld, margins = sp.spa_reference(codes, P, R, Wt, H, z_cutoff, sp.TOL_LD, 200, sp.LD)
    assert np.array_equal(f64, fld) and (f64 == 1).sum() >= least, np.bincount(f64.ravel())
    fin = np.isfinite(z64)
    assert not np.any(np.abs(np.abs(z64[fin]) - z_cutoff) <= 2.0 ** -40 * z_cutoff)
    m = np.array(margins)
    assert not np.any((m >= 2.0 ** -31) & (m <= 2.0 ** -29))
    assert max(e64.max(), eld.max()) <= 12
    ok = np.isfinite(pld.astype(np.float64)) & (pld > 1e-200)
    eps = float(np.abs(np.log(p64[ok].astype(sp.LD)) - np.log(pld[ok])).max())
    return _frozen(pld, f64) + (eps,)


@functools.lru_cache(maxsize=None)
def reference(indiv, snps, n, kh, z_cutoff):
    codes, _, _, _, P, R, Wt, H = case(indiv, snps, n, kh)
    return both_references(codes, P, R, Wt, H, z_cutoff, 5)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")


def _columns(M, ld, device):
    rows, cols = M.shape
    buf = np.full((max(cols, 1), ld), np.nan)
    buf[:cols, :rows] = M.T
    return _dev(buf) if device else buf


def run(mx, plink, P, R, Wt, H, z_cutoff=2.0, tol=TOL, max_iter=MAX_ITER, dev=False, ldo=None, want_flag=True, want_nobs=True, want=(True, True, True)):
    """one call through the C ABI, every operand and result on the host or on the device; returns a dict of (snps, n) arrays (None where not asked for) after
    checking that nothing beyond row snps - 1 of a column or beyond column n - 1 was written"""
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    indiv, n = R.shape
    snps = plink.shape[0]
    kh = H.shape[1] // n
    ldo = ldo or snps
    ld = indiv + 1
    new = lambda fill, dt=np.float64: (_dev(np.full((n + 1, ldo), fill, dt)) if dev else np.full((n + 1, ldo), fill, dt))          # noqa: E731
    res = [new(SENTINEL) if w else None for w in want] + [new(SENTINEL)]
    flag = new(-3, np.int32) if want_flag else None
    nobs = (_dev(np.full(snps + 1, -3, np.int32)) if dev else np.full(snps + 1, -3, np.int32)) if want_nobs else None
    X, pb, rb, wb, hb = _dev(plink) if dev else np.ascontiguousarray(plink), *(_columns(M, ld, dev) for M in (P, R, Wt, H))          # (alive until the call is over)
    rc = L.mxa_assoc_score_spa(p(X), snps, indiv, p(pb), ld, p(rb), ld, p(wb), ld, p(hb) if kh else None, ld, n, kh, float(z_cutoff), float(tol), int(max_iter),
                               p(res[0]), p(res[1]), p(res[2]), p(res[3]), ldo, p(flag), p(nobs))
    assert rc == 0, mx.lib.last_error()
    out = {}
    for name, r, fill in zip(("score", "var", "z", "pval", "flag"), res + [flag], (SENTINEL,) * 4 + (-3,)):
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


def same(a, b):
    """every array of two results bit for bit"""
    return all((a[k] is None and b[k] is None) or np.array_equal(op.bits(a[k]), op.bits(b[k])) for k in a)


def log_error(got, ref):
    """(the largest |log got - log ref| over the finite reference p-values above 1e-200, their number); NaNs must sit in the same places"""
    ref = np.asarray(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref.astype(np.float64)))
    ok = np.isfinite(ref.astype(np.float64)) & (ref > 1e-200)
    assert np.all(got[ok] > 0)
    return float(np.abs(np.log(got[ok].astype(sp.LD)) - np.log(ref[ok].astype(sp.LD))).max()), int(ok.sum())


@pytest.mark.parametrize("indiv, snps, n, kh, z_cutoff", CASES)
def test_flags_and_p_values_against_the_references(mx, indiv, snps, n, kh, z_cutoff):
    codes, plink, Y, W, P, R, Wt, H = case(indiv, snps, n, kh)
    pld, flags, eps = reference(indiv, snps, n, kh, z_cutoff)
    assert 0.02 < Y.mean() < 0.07 and np.any(codes < 0)
    got = run(mx, plink, P, R, Wt, H, z_cutoff)
    (score, var, z), nobs = run_score(mx, plink, R, Wt, H)
    for name, want in (("score", score), ("var", var), ("z", z), ("nobs", nobs)):
        assert np.array_equal(op.bits(got[name]), op.bits(want)), name
    assert np.array_equal(got["flag"], flags), np.argwhere(got["flag"] != flags)[:5]
    err, count = log_error(got["pval"], pld)
    bound = 16 * max(eps, 2.0 ** -48)
    print(f"indiv {indiv} snps {snps} n {n} kh {kh} z_cutoff {z_cutoff}: flags {np.bincount(flags.ravel(), minlength=4)}, eps {eps:.3g}, "
          f"max |log pval - log p_LD| {err:.3g} over {count} entries, bound {bound:.3g}, smallest p {float(np.nanmin(got['pval'])):.3g}")
    assert err <= bound
    # the same call with everything on the device: the same bits
    assert same(got, run(mx, plink, P, R, Wt, H, z_cutoff, dev=True))


@functools.lru_cache(maxsize=None)
def edge_case():
    """indiv 67, n = 1, kh = 0 (g = x): SNP 0 entirely missing (N = 0), SNP 1 monomorphic (no minor allele: U = V = 0 exactly), SNP 2 carried by two cases
    alone without a missing call (U = G+ - c0: the observed side on the edge of the support), then ordinary rows"""
    snps = 12
    codes, plink, Y, W, P, R, Wt, H = case(67, 33, 1, 0)
    codes = codes[:snps].copy()
    codes[0] = -1
    codes[1] = 0
    codes[2] = 0
    codes[2, np.flatnonzero(Y[:, 0] > 0)[:2]] = (1, 2)
    return _frozen(codes, sp.pack(codes)) + (P, R, Wt, H)


def test_edges_all_missing_monomorphic_and_the_edge_of_the_support(mx):
    codes, plink, P, R, Wt, H = edge_case()
    pld, flags, eps = both_references(codes, P, R, Wt, H, 1.0, 1)
    assert list(flags[:3, 0]) == [3, 3, 2] and set(flags[3:, 0]) <= {0, 1}
    bound = 16 * max(eps, 2.0 ** -48)
    for dev in (False, True):
        got = run(mx, plink, P, R, Wt, H, 1.0, dev=dev)
        assert np.array_equal(got["flag"], flags)
        assert np.isnan(got["pval"][0, 0]) and np.isnan(got["pval"][1, 0]) and abs(got["z"][2, 0]) > 2
        assert abs(math.log(got["pval"][2, 0]) - math.log(math.erfc(abs(got["z"][2, 0]) / math.sqrt(2.0)))) <= bound
        assert log_error(got["pval"], pld)[0] <= bound


def test_an_infinite_cutoff_corrects_nothing_and_one_evaluation_solves_nothing(mx):
    indiv, snps, n, kh, z_cutoff = CASES[1]
    codes, plink, Y, W, P, R, Wt, H = case(indiv, snps, n, kh)
    got = run(mx, plink, P, R, Wt, H, math.inf)
    (score, var, z), nobs = run_score(mx, plink, R, Wt, H)
    assert np.all(got["flag"] == 0) and np.array_equal(op.bits(got["z"]), op.bits(z)) and np.all(np.isfinite(z))
    normal = np.array([[math.erfc(abs(v) / math.sqrt(2.0)) for v in row] for row in z])
    assert log_error(got["pval"], normal)[0] <= 16 * 2.0 ** -48
    # max_iter = 1: every item that is to be corrected ends with the flag 2 and the normal p-value
    _, flags, _ = reference(indiv, snps, n, kh, z_cutoff)
    one = run(mx, plink, P, R, Wt, H, z_cutoff, max_iter=1)
    assert np.array_equal(one["flag"], np.where(flags == 1, 2, flags)) and (flags == 1).sum() >= 5
    assert np.array_equal(op.bits(one["pval"]), op.bits(got["pval"]))


def test_dirty_padding_larger_ldo_and_optional_outputs(mx):
    indiv, snps, n, kh, z_cutoff = CASES[1]
    codes, plink, Y, W, P, R, Wt, H = case(indiv, snps, n, kh)
    assert op.padding_fields(indiv) > 0
    plain = run(mx, plink, P, R, Wt, H, z_cutoff)
    for code in op.CODES:
        assert same(plain, run(mx, op.dirty(plink, indiv, code), P, R, Wt, H, z_cutoff, dev=code in (1, 3)))
    for dev in (False, True):
        assert same(plain, run(mx, plink, P, R, Wt, H, z_cutoff, dev=dev, ldo=snps + 5))
        part = run(mx, plink, P, R, Wt, H, z_cutoff, dev=dev, want_flag=False, want_nobs=False, want=(False, True, False))
        assert part["flag"] is None and "nobs" not in part and part["score"] is None and part["z"] is None
        assert np.array_equal(op.bits(part["pval"]), op.bits(plain["pval"])) and np.array_equal(op.bits(part["var"]), op.bits(plain["var"]))


@pytest.mark.parametrize("indiv, snps, n, kh, z_cutoff", [CASES[1], CASES[5]])
def test_chunks_batches_and_runs_give_the_same_bits(mx, monkeypatch, indiv, snps, n, kh, z_cutoff):
    codes, plink, Y, W, P, R, Wt, H = case(indiv, snps, n, kh)
    first = run(mx, plink, P, R, Wt, H, z_cutoff)
    assert same(first, run(mx, plink, P, R, Wt, H, z_cutoff))
    for name, value in (("MXA_ASSOC_CHUNK_ROWS", "7"), ("MXA_ASSOC_SPA_BATCH", "1"), ("MXA_ASSOC_SPA_BATCH", "5")):
        monkeypatch.setenv(name, value)
        for dev in (False, True):
            assert same(first, run(mx, plink, P, R, Wt, H, z_cutoff, dev=dev)), (name, value, dev)
        monkeypatch.delenv(name)


def test_mixed_sides_of_flag_and_pval_are_refused(mx):
    codes, plink, Y, W, P, R, Wt, H = case(*CASES[0][:4])
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    indiv, snps = CASES[0][:2]
    z, pv, fl = np.full((1, snps), SENTINEL), np.full((1, snps), SENTINEL), _dev(np.full((1, snps), -3, np.int32))
    zd = _dev(z)
    X, pb, rb, wb, hb = np.ascontiguousarray(plink), *(_columns(M, indiv, False) for M in (P, R, Wt, H))
    args = (p(X), snps, indiv, p(pb), indiv, p(rb), indiv, p(wb), indiv, p(hb), indiv, 1, 1, 2.0, TOL, MAX_ITER)
    assert L.mxa_assoc_score_spa(*args, None, None, p(z), p(pv), snps, p(fl), None) == 1 and L.mxa_last_error() == 1
    assert L.mxa_assoc_score_spa(*args, None, None, p(zd), p(pv), snps, None, None) == 1 and L.mxa_last_error() == 1
    assert np.all(z == SENTINEL) and np.all(pv == SENTINEL) and np.all(op.readback(fl) == -3)


def test_the_python_entries_end_to_end(mx):
    import torch
    indiv, snps, n, kh, z_cutoff = CASES[4]
    codes, plink, Y, W, P, R, Wt, H = case(indiv, snps, n, kh)
    pld, flags, eps = reference(indiv, snps, n, kh, z_cutoff)
    want = run(mx, plink, P, R, Wt, H, z_cutoff)
    full = mx.assoc_logistic(plink, snps, indiv, Y, covariates=W, spa=True, z_cutoff=z_cutoff)
    assert isinstance(full, mx.assoc.AssocSpaResult) and np.array_equal(full.flag, flags) and full.flag.dtype == np.int32
    assert log_error(full.pval, pld)[0] <= 16 * max(eps, 2.0 ** -48)
    direct = mx.assoc_score_spa(plink, snps, indiv, P, R, Wt, H, z_cutoff=z_cutoff)
    for a, b, key in zip(full, direct, full._fields):
        assert np.array_equal(op.bits(a), op.bits(b)) and np.array_equal(op.bits(a), op.bits(want[key])), key
    plain = mx.assoc_logistic(plink, snps, indiv, Y, covariates=W)
    assert isinstance(plain, mx.assoc.AssocScoreResult) and np.array_equal(op.bits(plain.z), op.bits(full.z))
    dev = mx.assoc_score_spa(_dev(plink), snps, indiv, *(torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (P, R, Wt, H)), z_cutoff=z_cutoff)
    assert dev.pval.is_cuda and dev.flag.is_cuda and dev.flag.dtype == torch.int32 and isinstance(dev.nobs, np.ndarray)
    for a, key in zip(dev[:5], dev._fields):
        assert np.array_equal(op.bits(op.readback(a)), op.bits(want[key])), key
    one = mx.assoc_logistic(plink, snps, indiv, Y[:, 0], covariates=W, spa=True, z_cutoff=z_cutoff, max_iter=40)
    assert one.pval.shape == (snps,) and one.flag.shape == (snps,) and np.array_equal(one.flag, flags[:, 0])
    out = {"pval": np.full((snps, n), SENTINEL, order="F"), "var": np.full((snps, n), SENTINEL, order="F")}
    res = mx.assoc_score_spa(plink, snps, indiv, P, R, Wt, H, z_cutoff=z_cutoff, out=out)
    assert res.pval is out["pval"] and res.var is out["var"] and res.z is None and res.score is None
    assert np.array_equal(op.bits(out["pval"]), op.bits(want["pval"])) and np.array_equal(op.bits(out["var"]), op.bits(want["var"]))
