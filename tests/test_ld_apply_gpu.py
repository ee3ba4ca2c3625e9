"""mxa_ld_window_apply / mxa_ld_window_apply_pairwise: Y = T_w(R) X, the window applied to a matrix without writing its rows.

T is formed in numpy (tests/_ld_apply_ref.py), in the kernel's operation order, from the BITS mxa_ld_window_rows(_pairwise) stores at kind 0 (N_ij: an exact
integer numpy product), so the apply kernels are tested apart from the r map.  u = 2^-53, m = last[i] - first[i] + 1.
  1. against the definition: |Y - fsum_j(T[i, j] X[j, c])| <= (m + 2) u sum_j |T[i, j] X[j, c]| -- m u sum|tx| bounds a length-m dot product in any order, with or
     without FMA (gamma_m to first order), one u sum|tx| covers the reference's own product roundings, one the 1 / (1 - m u) of gamma_m;
  2. unit columns, bit for bit: Y[i, k] == T[i, k] inside the window, 0.0 outside;
  3. n = 1, X = 1 against the scores entries: |Y - scores| <= 2 m u sum|t| (the same terms in two orders);
  4. the same bits from both engines, host and device X / Y, one tile row per group, two runs, and for every n (column c = the one-column call);
  5. errors: return 1, mxa_last_error() == 1, Y untouched;   6. the Python wrappers.
X is padded with NaN rows (ldx = snps + 5: never read), Y with sentinel rows (ldy = snps + 3) and a guard column behind column n - 1 (never written)."""
import numpy as np
import pytest

import _ld_apply_ref as ar
import _ld_ref as ref
from _util import make_problem, pack_plink, synth_genotypes

pytestmark = pytest.mark.gpu

U, NC = ar.U, ar.NC
SENTINEL = -12345.678
SHAPES = [(777, 515), (130, 1031), (1300, 67)]
NS = (1, 3, NC, NC + 1, 40, 2, 4, 7, 9, 15)
ROUTES = ("plain", "pairwise-missing", "pairwise-missing-free")
UNIT_COLUMNS = (0, 31, 32, 255, 256, 257, 511, 512, 699)


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    assert m.crossproduct.LD_APPLY_NC == NC
    return m


@pytest.fixture(autouse=True)
def _default_environment(monkeypatch):
    monkeypatch.delenv("MXA_XPROD_ENGINE", raising=False)
    monkeypatch.delenv("MXA_LD_PAIRWISE_SCRATCH_MB", raising=False)
    monkeypatch.delenv("MXA_LD_PAIRWISE_DENSE", raising=False)


# ------------------------------------------------------------------------------------------------------------------------------ data, windows
def _window_names(snps):
    names = [f"w={w}" for w in sorted({w for w in (0, 1, 255, 256, 257, snps - 1) if w < snps})] + ["chromosomes"]
    if snps >= 777:                                             # the cluster family's run of 600 SNPs from index 200 on
        names.append("clusters")
    return names + [f"sweep {s}" for s in range(3)]


def _window(snps, name):
    if name.startswith("w="):
        return ref.fixed_last(snps, int(name[2:]))
    if name == "chromosomes":
        return ar.chromosome_window(snps)
    if name == "clusters":
        return ar.cluster_window(snps)
    return ref.sweep_window(snps, int(name.split()[1]))


_CACHE = {}


def _case(snps, indiv, route):
    """dict(X packed, f or None, N or None); asserted on the reference side: no SNP is monomorphic (diag c > 0; pairwise: on its genotyped individuals)"""
    key = (snps, indiv, route)
    if key not in _CACHE:
        seed = snps + indiv
        if route == "plain":
            prob = make_problem(snps, indiv, 1, seed=seed)
            Z, f = prob["Z"].astype(np.float64), prob["f"]
            assert np.all((Z * Z).sum(axis=0) - 4.0 * indiv * f * f > 0)
            _CACHE[key] = dict(X=prob["plink"], f=f, N=None)
        else:
            Z, miss = synth_genotypes(snps, indiv, seed=seed, missing_frac=0.05 if route == "pairwise-missing" else 0.0)
            Zm = np.ma.masked_array(Z, mask=miss if miss is not None else False)
            assert np.all(Zm.max(axis=0) > Zm.min(axis=0))
            X = np.ascontiguousarray(pack_plink(Z.T.copy(), None if miss is None else miss.T.copy()))
            _CACHE[key] = dict(X=X, f=None, N=ar.present_counts(X, indiv))
    return _CACHE[key]


def _to(a, device):
    if a is None or not device:
        return a
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _suffix(route):
    return "" if route == "plain" else "_pairwise"


def _rows(mx, case, route, snps, indiv, last):
    """the kind-0 rows of the window as a dense symmetric matrix (NaN outside)"""
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    total = int(ref.rowptr_of(last)[-1])
    out = np.full(total + 7, SENTINEL)
    args = [p(case["X"]), snps, indiv, p(last), p(out), 0] + ([1, p(case["f"])] if route == "plain" else [])
    assert getattr(L, "mxa_ld_window_rows" + _suffix(route))(*args) == 0, mx.lib.last_error()
    assert np.all(out[total:] == SENTINEL)
    return ar.dense(out[:total], last)


def _terms(R, case, route, indiv, term):
    T = ar.terms(R, indiv, term) if route == "plain" else ar.terms_pw(R, case["N"], term)
    return T


def _raw(mx, case, route, snps, indiv, last, term, Xp, ldx, n, Yp, ldy):
    """the C entry on prepared buffers; returns (rc, error code)"""
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    args = [p(case["X"]), snps, indiv, p(last), term, p(Xp), ldx, n, p(Yp), ldy] + ([1, p(case["f"])] if route == "plain" else [])
    rc = getattr(L, "mxa_ld_window_apply" + _suffix(route))(*args)
    return rc, L.mxa_last_error()


def _apply(mx, case, route, snps, indiv, last, term, Xm, device=False, pad=True):
    """Y (snps x n) of the call on the n columns of Xm, from padded buffers: ldx = snps + 5 (NaN rows), ldy = snps + 3 and one guard column (sentinels)"""
    n = Xm.shape[1]
    ldx, ldy = (snps + 5, snps + 3) if pad else (snps, snps)
    Xp = np.full((n, ldx), np.nan)
    Xp[:, :snps] = Xm.T
    Yp = np.full((n + 1, ldy), SENTINEL)
    Xd, Yd = _to(Xp, device), _to(Yp, device)
    rc, err = _raw(mx, case, route, snps, indiv, last, term, Xd, ldx, n, Yd, ldy)
    assert (rc, err) == (0, 0), mx.lib.last_error()
    if device:
        import torch
        torch.cuda.synchronize()
        Yd = Yd.cpu().numpy()
    assert np.all(Yd[:n, snps:] == SENTINEL) and np.all(Yd[n] == SENTINEL), "written outside Y"
    return np.ascontiguousarray(Yd[:n, :snps].T)


def _x(snps, n=40, seed=5):
    return np.random.default_rng([snps, seed]).standard_normal((snps, n))


# ---------------------------------------------------------------------------------------------------------------- 1. against the definition
DEFINITION_CASES = [(s, k, r, w) for s, k in SHAPES for r in ROUTES for w in _window_names(s)]


@pytest.mark.parametrize("term", (0, 1, 2), ids=ar.TERMS)
@pytest.mark.parametrize("snps,indiv,route,window", DEFINITION_CASES)
def test_apply_is_the_windowed_product_within_the_summation_bound(mx, snps, indiv, route, window, term):
    case = _case(snps, indiv, route)
    last = _window(snps, window)
    T = _terms(_rows(mx, case, route, snps, indiv, last), case, route, indiv, term)
    Xm = _x(snps)
    want, mag, m = ar.apply_ref(T, last, Xm)                     # the n-column call's reference is the first n columns of this one
    assert np.isfinite(want).all()
    bound = (m[:, None] + 2.0) * U * mag
    worst = 0.0
    for n in NS:
        Y = _apply(mx, case, route, snps, indiv, last, term, Xm[:, :n])
        err = np.abs(Y - want[:, :n])
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = float(np.nanmax(np.where(err > 0, err / bound[:, :n], 0.0)))
        worst = max(worst, ratio)
        assert np.all(err <= bound[:, :n]), (n, ratio)
    print(f"apply {route} {snps}x{indiv} {window} {ar.TERMS[term]}: worst |err| / bound = {worst:.3f}, terms per SNP {int(m.min())} .. {int(m.max())}")


# ----------------------------------------------------------------------------------------------------------------------- 2. unit columns
@pytest.mark.parametrize("route", ROUTES)
def test_unit_columns_return_the_terms_bit_for_bit(mx, route):
    snps, indiv = 700, 131
    case = _case(snps, indiv, route)
    last = ar.cluster_window(snps)
    first = ref.first_of(last)
    R = _rows(mx, case, route, snps, indiv, last)
    E = np.zeros((snps, len(UNIT_COLUMNS)))
    E[list(UNIT_COLUMNS), np.arange(len(UNIT_COLUMNS))] = 1.0
    i = np.arange(snps)
    for term in (0, 1, 2):
        T = _terms(R, case, route, indiv, term)
        Y = _apply(mx, case, route, snps, indiv, last, term, E)
        for c, k in enumerate(UNIT_COLUMNS):
            inside = (first <= k) & (k <= last)
            assert inside.sum() >= 1 and np.isfinite(T[inside, k]).all()
            assert np.array_equal(Y[inside, c], T[inside, k]), (term, k, i[inside][Y[inside, c] != T[inside, k]][:5])
            assert np.all(Y[~inside, c] == 0.0), (term, k, i[~inside][Y[~inside, c] != 0.0][:5])


# ----------------------------------------------------------------------------------------------------------------------------- 3. scores
@pytest.mark.parametrize("route", ROUTES)
def test_one_column_of_ones_is_the_scores_within_two_summation_bounds(mx, route):
    snps, indiv = 777, 515
    case = _case(snps, indiv, route)
    cp = mx.crossproduct
    ones = np.ones((snps, 1))
    for last in (ar.cluster_window(snps), ref.sweep_window(snps, 1), ref.fixed_last(snps, 256)):
        R = _rows(mx, case, route, snps, indiv, last)
        for term in (1, 2):
            if route == "plain":
                S = cp.ld_window_scores(case["X"], snps, indiv, last, adjust=term == 2, is_plink_format=True, allele_freq=case["f"])
            else:
                S = cp.ld_window_scores_pairwise(case["X"], snps, indiv, last, adjust=term == 2)
            Y = _apply(mx, case, route, snps, indiv, last, term, ones)[:, 0]
            _, mag, m = ar.apply_ref(_terms(R, case, route, indiv, term), last, ones)
            err, bound = np.abs(Y - S), 2.0 * m * U * mag[:, 0]
            print(f"apply against scores {route} term {term}: worst |err| / bound = {float((err / bound).max()):.3f}")
            assert np.all(err <= bound)


# ------------------------------------------------------------------------------------------------------------------------- 4. invariance
@pytest.mark.parametrize("route", ROUTES)
def test_the_bits_do_not_depend_on_engine_pointers_groups_runs_or_n(mx, monkeypatch, route):
    snps, indiv = 777, 515
    case = _case(snps, indiv, route)
    last = ref.sweep_window(snps, 2)
    Xm = _x(snps)
    for term in (0, 2):
        base = _apply(mx, case, route, snps, indiv, last, term, Xm)
        assert np.isfinite(base).all()
        assert np.array_equal(_apply(mx, case, route, snps, indiv, last, term, Xm), base), "run to run"
        assert np.array_equal(_apply(mx, case, route, snps, indiv, last, term, Xm, device=True), base), "device X / Y"
        monkeypatch.setenv("MXA_XPROD_ENGINE", "i8")
        assert np.array_equal(_apply(mx, case, route, snps, indiv, last, term, Xm), base), "int8 engine"
        monkeypatch.delenv("MXA_XPROD_ENGINE")
        monkeypatch.setenv("MXA_LD_PAIRWISE_SCRATCH_MB", "1")     # one tile row per group
        assert np.array_equal(_apply(mx, case, route, snps, indiv, last, term, Xm), base), "one tile row per group"
        monkeypatch.delenv("MXA_LD_PAIRWISE_SCRATCH_MB")
        for c in (0, NC - 1, NC, 39):
            one = _apply(mx, case, route, snps, indiv, last, term, Xm[:, c: c + 1])
            assert np.array_equal(one[:, 0], base[:, c]), ("column alone", c)


# ----------------------------------------------------------------------------------------------------------------------------- 5. errors
def test_bad_arguments_return_one_and_leave_y_untouched(mx):
    snps, indiv, n = 300, 40, 3
    prob = make_problem(snps, indiv, 1, seed=9)
    plain = dict(X=prob["plink"], f=prob["f"])
    two = dict(X=np.ascontiguousarray(prob["plink"][:, :1]), f=prob["f"])     # 2 individuals: one byte per SNP
    good = ref.fixed_last(snps, 10)
    decreasing = good.copy()
    decreasing[7] = 30
    Xp = np.ones((n, snps))
    bad = (1, 1, True)

    def run(route, case=plain, nind=indiv, last=good, term=1, x=Xp, ldx=snps, cols=n, with_y=True, ldy=snps):
        Y = np.full((n + 1) * snps, SENTINEL)
        rc, err = _raw(mx, case, route, snps, nind, last, term, x, ldx, cols, Y if with_y else None, ldy)
        return rc, err, bool(np.all(Y == SENTINEL))

    for route in ("plain", "pairwise-missing"):
        assert run(route, cols=0) == bad, route
        assert run(route, ldx=snps - 1) == bad and run(route, ldy=snps - 1) == bad, route
        assert run(route, term=3) == bad and run(route, term=-1) == bad, route
        assert run(route, case=two, nind=2, term=2) == bad, route
        assert run(route, x=None) == bad and run(route, with_y=False) == bad, route
        assert run(route, last=decreasing) == bad and run(route, last=None) == bad, route
        assert run(route) == (0, 0, False), route                                  # the process is alive and the next good call succeeds
    assert run("plain", case=dict(X=plain["X"], f=None)) == bad


# ------------------------------------------------------------------------------------------------------------------- 6. Python wrappers
def test_python_wrappers(mx):
    import torch
    snps, indiv = 777, 515
    case = _case(snps, indiv, "plain")
    cp = mx.crossproduct
    X, f = case["X"], case["f"]
    Xm = _x(snps, n=3)
    kw = dict(is_plink_format=True, allele_freq=f)
    Y = cp.ld_window_apply(X, snps, indiv, Xm, window=40, term="r", **kw)
    assert isinstance(Y, np.ndarray) and Y.shape == (snps, 3)
    assert np.array_equal(Y, cp.ld_window_apply(X, snps, indiv, Xm, last=ref.fixed_last(snps, 40), term="r", **kw))      # window= against last=
    assert np.array_equal(Y, _apply(mx, case, "plain", snps, indiv, ref.fixed_last(snps, 40), 0, Xm))
    y1 = cp.ld_window_apply(X, snps, indiv, Xm[:, 1], window=40, term="r", **kw)                                          # 1-D X: one column
    assert y1.shape == (snps,) and np.array_equal(y1, Y[:, 1])
    dev = torch.device("cuda", 0)
    Yd = cp.ld_window_apply(torch.from_numpy(X).to(dev), snps, indiv, torch.from_numpy(Xm).to(dev), window=40, term="r", is_plink_format=True,
                            allele_freq=torch.from_numpy(f).to(dev))
    assert Yd.is_cuda and tuple(Yd.shape) == (snps, 3) and np.array_equal(Yd.cpu().numpy(), Y)
    out = np.zeros((snps, 3), order="F")
    assert cp.ld_window_apply(X, snps, indiv, Xm, window=40, term="r", out=out, **kw) is out and np.array_equal(out, Y)
    ones = np.ones((snps, 1))
    for adjust, term in ((False, "r2"), (True, "r2_adj")):
        P = cp.ld_scores_partitioned(X, snps, indiv, ones, window=40, adjust=adjust, **kw)
        assert np.array_equal(P, cp.ld_window_apply(X, snps, indiv, ones, window=40, term=term, **kw))
    casep = _case(snps, indiv, "pairwise-missing")
    Pp = cp.ld_scores_partitioned(casep["X"], snps, indiv, ones, window=40, pairwise=True)
    assert np.array_equal(Pp, cp.ld_window_apply(casep["X"], snps, indiv, ones, window=40, term="r2", pairwise=True))
