"""The LD operator object (mxa_ld_op_*): the window's values staged once on the device, applied and ridge-solved there.  u = 2^-53, m = last - first + 1.
  1. exact: from_rows on dyadic rows, small integer X, shift in {0, 0.5, -2}: Y equals numpy's product bit for bit (every partial sum is representable in any
     order); unit columns return T[:, k] + shift e_k and 0.0 outside the window; mxa_ld_op_rows returns the input bits;
  2. creation: mxa_ld_op_rows equals mxa_ld_window_rows(_pairwise) bit for bit on the plain, pairwise-missing and pairwise-missing-free routes at kind 0 and 1,
     and under MXA_XPROD_ENGINE=i8;
  3. definition: |Y - fsum_j T[i, j] X[j, c] - shift X[i, c]| <= (m + 3) u (sum_j |T X| + |shift X[i, c]|) -- test_ld_apply_gpu.py's bound plus one term for
     the shift; at shift 0 against mxa_ld_window_apply term 0 / 1: <= 2 (m + 2) u sum |T X| (the same terms in two orders);
  4. the same bits across two runs, host and device X / Y, every n (column c = the one-column call), create against from_rows on the exported rows;
  5. solve at tol = 1e-10: status, relres, the true residual in long double (<= 2 tol), iters <= numpy's + 2, on every window family of the three shapes
     ((1300, 67): kind 1 at shift 2 only) and of the dyadic family; w = 0: one iteration; a zero column; max_iter = 3 (the iterate against numpy's and its
     residual against the recurrence's);
     breakdown on the indefinite (1300, 67) w = 255 kind 0 shift 0.5; column independence bit for bit; host against device B / X;
  6. errors: return 1, mxa_last_error() == 1, outputs and sentinels untouched, *op NULL; free twice; use after free;
  7. the Python class.
X is padded with NaN rows (ldx = snps + 5: never read), Y with sentinel rows (ldy = snps + 3) and a guard column behind column n - 1 (never written)."""
import ctypes

import numpy as np
import pytest

import _ld_apply_ref as ar
import _ld_op_ref as opr
import _ld_ref as ref
from _util import make_problem, pack_plink, synth_genotypes

pytestmark = pytest.mark.gpu

U = opr.U
SENTINEL = -12345.678
SHAPES = [(777, 515), (130, 1031), (1300, 67)]
NS = (1, 3, 16, 17, 40, 2, 4, 7, 9, 15)           # every kernel of apply_device: <1, 8>, <2, 8>, <4, 4> partial and full, <8, 4> and <16, 4> partial and full
ROUTES = ("plain", "pairwise-missing", "pairwise-missing-free")
UNIT_COLUMNS = (0, 31, 32, 255, 256, 257, 511, 512, 699)
SHIFTS = (0.0, 0.5, -2.0)
TOL = 1e-10


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


@pytest.fixture(autouse=True)
def _default_environment(monkeypatch):
    monkeypatch.delenv("MXA_XPROD_ENGINE", raising=False)
    monkeypatch.delenv("MXA_LD_PAIRWISE_SCRATCH_MB", raising=False)
    monkeypatch.delenv("MXA_LD_PAIRWISE_DENSE", raising=False)


# ------------------------------------------------------------------------------------------------------------------------------ data, windows
def _window_names(snps):
    names = [f"w={w}" for w in sorted({w for w in (0, 1, 255, 256, 257, snps - 1) if w < snps})] + ["chromosomes"]
    if snps >= 777:
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
    """dict(X packed, f or None): the data of test_ld_apply_gpu.py (no SNP is monomorphic)"""
    key = (snps, indiv, route)
    if key not in _CACHE:
        seed = snps + indiv
        if route == "plain":
            prob = make_problem(snps, indiv, 1, seed=seed)
            Z, f = prob["Z"].astype(np.float64), prob["f"]
            assert np.all((Z * Z).sum(axis=0) - 4.0 * indiv * f * f > 0)
            _CACHE[key] = dict(X=prob["plink"], f=f)
        else:
            Z, miss = synth_genotypes(snps, indiv, seed=seed, missing_frac=0.05 if route == "pairwise-missing" else 0.0)
            Zm = np.ma.masked_array(Z, mask=miss if miss is not None else False)
            assert np.all(Zm.max(axis=0) > Zm.min(axis=0))
            _CACHE[key] = dict(X=np.ascontiguousarray(pack_plink(Z.T.copy(), None if miss is None else miss.T.copy())), f=None)
    return _CACHE[key]


def _to(a, device):
    if a is None or not device:
        return a
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _suffix(route):
    return "" if route == "plain" else "_pairwise"


class Op:
    """a handle of the C ABI with its window; freed on exit"""

    def __init__(self, mx, handle, last):
        self.mx, self.h, self.last, self.snps = mx, handle, last, len(last)
        self.total = int(ref.rowptr_of(last)[-1])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.mx.lib.check_library_handle().mxa_ld_op_free(ctypes.byref(self.h))
        assert not self.h.value
        return False

    def rows(self, device=False):
        L, p = self.mx.lib.check_library_handle(), self.mx.lib.ptr
        out = _to(np.full(self.total + 7, SENTINEL), device)
        assert L.mxa_ld_op_rows(self.h, p(out)) == 0, self.mx.lib.last_error()
        if device:
            out = out.cpu().numpy()
        assert np.all(out[self.total:] == SENTINEL)
        return out[:self.total]

    def apply(self, Xm, shift=0.0, device=False, device_y=None):
        """Y (snps x n) from padded buffers: ldx = snps + 5 (NaN rows), ldy = snps + 3 and one guard column (sentinels)"""
        L, p = self.mx.lib.check_library_handle(), self.mx.lib.ptr
        snps, n = self.snps, Xm.shape[1]
        ldx, ldy = snps + 5, snps + 3
        Xp = np.full((n, ldx), np.nan)
        Xp[:, :snps] = Xm.T
        Yp = np.full((n + 1, ldy), SENTINEL)
        device_y = device if device_y is None else device_y
        Xd, Yd = _to(Xp, device), _to(Yp, device_y)
        rc = L.mxa_ld_op_apply(self.h, shift, p(Xd), ldx, n, p(Yd), ldy)
        assert (rc, L.mxa_last_error()) == (0, 0), self.mx.lib.last_error()
        if device_y:
            import torch
            torch.cuda.synchronize()
            Yd = Yd.cpu().numpy()
        assert np.all(Yd[:n, snps:] == SENTINEL) and np.all(Yd[n] == SENTINEL), "written outside Y"
        return np.ascontiguousarray(Yd[:n, :snps].T)

    def solve(self, Bm, shift, tol=TOL, max_iter=1000, device=False):
        """(X, iters, relres, status, rc) from padded buffers: ldb = snps + 5 (NaN rows), ldx = snps + 3 and a guard column"""
        L, p = self.mx.lib.check_library_handle(), self.mx.lib.ptr
        snps, n = self.snps, Bm.shape[1]
        ldb, ldx = snps + 5, snps + 3
        Bp = np.full((n, ldb), np.nan)
        Bp[:, :snps] = Bm.T
        Xp = np.full((n + 1, ldx), SENTINEL)
        Bd, Xd = _to(Bp, device), _to(Xp, device)
        iters, relres, status = np.full(n + 1, -7, np.int32), np.full(n + 1, SENTINEL), np.full(n + 1, -7, np.int32)
        rc = L.mxa_ld_op_solve(self.h, shift, p(Bd), ldb, n, p(Xd), ldx, tol, max_iter, p(iters), p(relres), p(status))
        assert (rc, L.mxa_last_error()) == (0, 0), self.mx.lib.last_error()
        if device:
            import torch
            torch.cuda.synchronize()
            Xd = Xd.cpu().numpy()
        assert np.all(Xd[:n, snps:] == SENTINEL) and np.all(Xd[n] == SENTINEL), "written outside X"
        assert iters[n] == -7 and relres[n] == SENTINEL and status[n] == -7
        return np.ascontiguousarray(Xd[:n, :snps].T), iters[:n].copy(), relres[:n].copy(), status[:n].copy()


def _from_rows(mx, last, rows, device=False):
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    h = ctypes.c_void_p(None)
    rows = _to(np.ascontiguousarray(rows), device)
    assert L.mxa_ld_op_from_rows(len(last), p(last), p(rows), ctypes.byref(h)) == 0, mx.lib.last_error()
    assert h.value
    return Op(mx, h, last)


def _create(mx, case, route, snps, indiv, last, kind):
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    h = ctypes.c_void_p(None)
    if route == "plain":
        rc = L.mxa_ld_op_create(p(case["X"]), snps, indiv, p(last), kind, 1, p(case["f"]), ctypes.byref(h))
    else:
        rc = L.mxa_ld_op_create_pairwise(p(case["X"]), snps, indiv, p(last), kind, ctypes.byref(h))
    assert rc == 0 and h.value, mx.lib.last_error()
    return Op(mx, h, last)


def _window_rows(mx, case, route, snps, indiv, last, kind):
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    total = int(ref.rowptr_of(last)[-1])
    out = np.full(total, SENTINEL)
    args = [p(case["X"]), snps, indiv, p(last), p(out), kind] + ([1, p(case["f"])] if route == "plain" else [])
    assert getattr(L, "mxa_ld_window_rows" + _suffix(route))(*args) == 0, mx.lib.last_error()
    return out


def _window_apply(mx, case, route, snps, indiv, last, term, Xm):
    cp = mx.crossproduct
    kw = dict(pairwise=True) if route != "plain" else dict(is_plink_format=True, allele_freq=case["f"])
    return cp.ld_window_apply(case["X"], snps, indiv, Xm, last=last, term=ar.TERMS[term], **kw)


def _x(snps, n=40, seed=5):
    return np.random.default_rng([snps, seed]).standard_normal((snps, n))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("snps,name", [(s, w) for s, _ in SHAPES for w in _window_names(s)])
def test_dyadic_rows_give_numpys_product_bit_for_bit(mx, snps, name):
    Xi = np.random.default_rng([snps, 1]).integers(-4, 5, (snps, 40)).astype(np.float64)
    last = _window(snps, name)
    rows = opr.dyadic_rows(last)
    W = opr.windowed(ar.dense(rows, last), last)
    with _from_rows(mx, last, rows) as op:
        assert np.array_equal(_bits(op.rows()), _bits(rows))
        assert np.array_equal(_bits(op.rows(device=True)), _bits(rows))
        for shift in SHIFTS:
            want = opr.apply_exact(W, Xi, shift)
            for n in NS:
                Y = op.apply(Xi[:, :n], shift)
                assert np.array_equal(Y, want[:, :n]), (shift, n, np.argwhere(Y != want[:, :n])[:3])


def test_unit_columns_return_the_terms_and_zero_outside_the_window(mx):
    snps = 777
    cols = [k for k in UNIT_COLUMNS if k < snps]
    E = np.zeros((snps, len(cols)))
    E[cols, np.arange(len(cols))] = 1.0
    for name in ("clusters", "sweep 1", "w=256"):
        last = _window(snps, name)
        first = ref.first_of(last)
        rows = opr.dyadic_rows(last)
        T = ar.dense(rows, last)
        with _from_rows(mx, last, rows, device=True) as op:
            for shift in SHIFTS:
                Y = op.apply(E, shift)
                for c, k in enumerate(cols):
                    ins = (first <= k) & (k <= last)
                    want = T[ins, k] + shift * (np.arange(snps)[ins] == k)
                    assert np.array_equal(Y[ins, c], want), (name, shift, k)
                    assert np.all(Y[~ins, c] == 0.0), (name, shift, k)


def test_a_nan_in_t_makes_exactly_the_rows_whose_window_holds_it_nan(mx):
    snps = 777
    last = _window(snps, "sweep 2")
    rows = opr.dyadic_rows(last)
    ii, jj = ref.pairs(last)
    e = int(np.flatnonzero((ii == 300) & (jj > 300))[0]) if np.any((ii == 300) & (jj > 300)) else int(np.flatnonzero(ii == 300)[0])
    rows[e] = np.nan
    i, j = int(ii[e]), int(jj[e])
    X = np.zeros((snps, 2))                                              # zeros: the NaN still shows (never skipped inside the window)
    X[:, 1] = 1.0
    with _from_rows(mx, last, rows) as op:
        Y = op.apply(X, 0.5)
    bad = np.zeros(snps, bool)
    bad[[i, j]] = True
    assert np.isnan(Y[bad]).all() and np.isfinite(Y[~bad]).all()


# --------------------------------------------------------------------------------------------------------------------------------- 2. creation
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("snps,indiv", SHAPES)
def test_create_stores_the_bits_of_the_rows_entries(mx, monkeypatch, snps, indiv, route):
    case = _case(snps, indiv, route)
    for name in _window_names(snps):
        last = _window(snps, name)
        for kind in (0, 1):
            want = _window_rows(mx, case, route, snps, indiv, last, kind)
            with _create(mx, case, route, snps, indiv, last, kind) as op:
                assert np.array_equal(_bits(op.rows()), _bits(want)), (name, kind)
            monkeypatch.setenv("MXA_XPROD_ENGINE", "i8")
            with _create(mx, case, route, snps, indiv, last, kind) as op:
                assert np.array_equal(_bits(op.rows(device=True)), _bits(want)), (name, kind, "int8 engine")
            monkeypatch.delenv("MXA_XPROD_ENGINE")


# ------------------------------------------------------------------------------------------------------------------------------- 3. definition
DEFINITION_CASES = [(s, k, r, w) for s, k in SHAPES for r in ROUTES for w in _window_names(s)]


@pytest.mark.parametrize("snps,indiv,route,window", DEFINITION_CASES)
def test_apply_is_the_windowed_product_within_the_summation_bound(mx, snps, indiv, route, window):
    case = _case(snps, indiv, route)
    last = _window(snps, window)
    Xm = _x(snps)
    for kind in (0, 1):
        with _create(mx, case, route, snps, indiv, last, kind) as op:
            T = ar.dense(op.rows(), last)
            want, mag, m = ar.apply_ref(T, last, Xm)                    # fsum of the float64 products, sum |T X| (a little below the true sum), m
            assert np.isfinite(want).all()
            worst = 0.0
            for shift in SHIFTS:
                full = (want.astype(opr.LD) + opr.LD(shift) * Xm.astype(opr.LD))
                bound = (m[:, None] + 3.0) * U * (mag + np.abs(shift * Xm) * (1.0 - 2.0 ** -40))
                for n in NS:
                    Y = op.apply(Xm[:, :n], shift)
                    err = np.abs(Y.astype(opr.LD) - full[:, :n]).astype(np.float64)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        worst = max(worst, float(np.nanmax(np.where(err > 0, err / bound[:, :n], 0.0))))
                    assert np.all(err <= bound[:, :n]), (kind, shift, n, worst)
            # the same terms in two orders: the entry that forms r^ anew on every call
            Y0 = op.apply(Xm, 0.0)
            Ya = _window_apply(mx, case, route, snps, indiv, last, kind, Xm)
            err2, bound2 = np.abs(Y0 - Ya), 2.0 * (m[:, None] + 2.0) * U * mag
            print(f"ld_op apply {route} {snps}x{indiv} {window} kind {kind}: worst |err| / bound = {worst:.3f}, against ld_window_apply "
                  f"{float((err2 / bound2).max()):.3f}, terms per SNP {int(m.min())} .. {int(m.max())}")
            assert np.all(err2 <= bound2), kind


# -------------------------------------------------------------------------------------------------------------------------------- 4. same bits
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("snps,indiv", SHAPES)
def test_the_bits_do_not_depend_on_runs_pointers_n_or_the_way_of_creation(mx, snps, indiv, route):
    case = _case(snps, indiv, route)
    last = ref.sweep_window(snps, 2)
    Xm = _x(snps)
    for kind in (0, 1):
        with _create(mx, case, route, snps, indiv, last, kind) as op:
            base = op.apply(Xm, 0.5)
            assert np.isfinite(base).all()
            assert np.array_equal(op.apply(Xm, 0.5), base), "run to run"
            assert np.array_equal(op.apply(Xm, 0.5, device=True), base), "device X / Y"
            assert np.array_equal(op.apply(Xm, 0.5, device=True, device_y=False), base), "device X, host Y"
            assert np.array_equal(op.apply(Xm, 0.5, device=False, device_y=True), base), "host X, device Y"
            for n in NS:
                assert np.array_equal(op.apply(Xm[:, :n], 0.5), base[:, :n]), ("the first n columns", n)
            for c in (0, 15, 16, 39):
                assert np.array_equal(op.apply(Xm[:, c: c + 1], 0.5)[:, 0], base[:, c]), ("column alone", c)
            with _from_rows(mx, last, op.rows()) as twin:
                assert np.array_equal(twin.apply(Xm, 0.5), base), "from_rows on the exported rows"


# ------------------------------------------------------------------------------------------------------------------------------------ 5. solve
def _rhs(snps, W, seed=7):
    """five columns that stop at different iterations: noise, zero, a unit vector, one eigenvector of W (one iteration), a sum of four eigenvectors (four)"""
    rng = np.random.default_rng([snps, seed])
    _, V = np.linalg.eigh(W)
    B = np.zeros((snps, 5))
    B[:, 0] = rng.standard_normal(snps)
    B[snps // 2, 2] = 3.0
    B[:, 3] = V[:, snps // 3]
    B[:, 4] = V[:, [0, snps // 4, snps // 2, snps - 1]] @ np.array([1.0, -2.0, 0.5, 1.5])
    return B


def _check_converged(op, W, shift, B, label):
    X, iters, relres, status = op.solve(B, shift)
    true = opr.true_relres(W, shift, X, B)
    for c in range(B.shape[1]):
        x_ref, it_ref, _, st_ref = opr.cg(W, shift, B[:, c], TOL, 1000)
        assert st_ref == 0, (label, c, "the reference did not converge")
        print(f"ld_op solve {label} column {c}: iters {iters[c]} (numpy {it_ref}), relres {relres[c]:.3e}, true {true[c]:.3e}")
        assert status[c] == 0 and relres[c] <= TOL, (label, c, status[c], relres[c])
        if np.any(B[:, c] != 0):
            assert true[c] <= 2 * TOL, (label, c, true[c])
            assert 1 <= iters[c] <= it_ref + 2, (label, c, iters[c], it_ref)
        else:
            assert iters[c] == 0 and relres[c] == 0.0 and np.all(X[:, c] == 0.0), (label, c)
    return X, iters, relres, status


SOLVE_CASES = [(s, k, w) for s, k in SHAPES for w in _window_names(s)]


@pytest.mark.parametrize("snps,indiv,window", SOLVE_CASES)
def test_solve_converges_on_the_ridge_systems(mx, snps, indiv, window):
    case = _case(snps, indiv, "plain")
    last = _window(snps, window)
    # (1300, 67): 67 individuals leave r^ far from positive definite once it is cut to a window (the breakdown test below); r^2 at shift 2 is the system to solve
    kinds, shifts = ((0, 1), (0.5, 2.0)) if (snps, indiv) != (1300, 67) else ((1,), (2.0,))
    for kind in kinds:
        with _create(mx, case, "plain", snps, indiv, last, kind) as op:
            W = opr.windowed(ar.dense(op.rows(), last), last)
            B = _rhs(snps, W)
            for shift in shifts:
                _, iters, _, _ = _check_converged(op, W, shift, B, f"{snps}x{indiv} {window} kind {kind} shift {shift}")
                if window == "w=0":                                      # T = I: (1 + shift) x = b, one iteration
                    assert np.all(iters[[0, 2, 3, 4]] == 1), iters


@pytest.mark.parametrize("window", _window_names(777))
def test_solve_converges_on_the_dyadic_family(mx, window):
    snps = 777
    last = _window(snps, window)
    rows = opr.decay_rows(last)
    W = opr.windowed(ar.dense(rows, last), last)
    with _from_rows(mx, last, rows) as op:
        _check_converged(op, W, 1.5, _rhs(snps, W), f"decay {window} shift 1.5")


def test_max_iter_leaves_the_third_iterate_and_status_one(mx):
    snps, indiv = 777, 515
    case = _case(snps, indiv, "plain")
    last = _window(snps, "w=256")
    with _create(mx, case, "plain", snps, indiv, last, 0) as op:
        W = opr.windowed(ar.dense(op.rows(), last), last)
        B = _rhs(snps, W)[:, [0, 2]]
        X, iters, relres, status = op.solve(B, 0.5, max_iter=3)
        ev = np.linalg.eigvalsh(W + 0.5 * np.eye(snps))
        kappa = ev.max() / ev.min()
        m = float((last - ref.first_of(last) + 1).max())
        for c in range(2):
            x_ref, it_ref, rel_ref, st_ref = opr.cg(W, 0.5, B[:, c], TOL, 3)
            assert (it_ref, st_ref) == (3, 1) and opr.cg(W, 0.5, B[:, c], TOL, 1000)[1] > 3
            assert (iters[c], status[c]) == (3, 1)
            # Three updates, each built from one apply (the definition's bound: (m + 3) u relative to sum |T p|) and two dot products of snps terms (snps u each,
            # any order); the scalars alpha and beta carry those relative errors into the iterate, the conditioning of the system amplifies them by at most kappa.
            # 8 per update covers the apply, both dot products, the two quotients and the two axpys on either side of the comparison.
            tol = 8 * 3 * kappa * (snps + m + 3) * U * np.abs(x_ref).max()
            print(f"ld_op solve max_iter 3 column {c}: max |x - numpy| = {np.abs(X[:, c] - x_ref).max():.3e}, allowed {tol:.3e}, relres {relres[c]:.3e} ({rel_ref:.3e})")
            assert np.abs(X[:, c] - x_ref).max() <= tol
            # No condition number in this one: the recurrence residual against b - A x of the returned iterate.  They start equal (x = 0, r = b).  A step adds
            # alpha p to x and takes alpha A p from r; with |alpha p| <= 2 |x| (CG's iterates grow in norm from 0) the roundings of the step move b - A x by at
            # most 3 u |A| |x| and r by u |r| + 2 u |A| |x| + 2 (m + 3) u | |A| | |x| (the product, the sum, and the apply's own (m + 3) u relative to |A| |p|):
            # (2 m + 11) u | |A| | |x| + u |b| per step in norm, | |A| | the 2-norm of the matrix of absolute values, |x| the returned iterate's.  relres itself
            # carries the snps u of its dot product.  A reduction or an alpha that is wrong beyond rounding moves x and not r's recurrence, or the reverse.
            A = W + 0.5 * np.eye(snps)
            res = (B[:, c].astype(opr.LD) - A.astype(opr.LD) @ X[:, c].astype(opr.LD)).astype(np.float64)
            nb = np.linalg.norm(B[:, c])
            gap = abs(np.linalg.norm(res) / nb - relres[c])
            allowed = 3 * ((2 * m + 11) * U * np.linalg.norm(np.abs(A), 2) * np.linalg.norm(X[:, c]) + U * nb) / nb + snps * U * relres[c]
            print(f"ld_op solve max_iter 3 column {c}: | |b - A x| / |b| - relres | = {gap:.3e}, allowed {allowed:.3e}")
            assert gap <= allowed
        X0, it0, _, st0 = op.solve(B, 0.5, max_iter=0)
        assert np.all(X0 == 0.0) and np.all(it0 == 0) and np.all(st0 == 1)


def test_an_indefinite_system_breaks_down_with_status_two(mx):
    snps, indiv = 1300, 67
    case = _case(snps, indiv, "plain")
    last = _window(snps, "w=255")
    with _create(mx, case, "plain", snps, indiv, last, 0) as op:
        W = opr.windowed(ar.dense(op.rows(), last), last)
        assert np.linalg.eigvalsh(W + 0.5 * np.eye(snps)).min() < -1.0
        B = _rhs(snps, W)[:, [0, 1]]
        assert opr.cg(W, 0.5, B[:, 0], TOL, 1000)[3] == 2
        X, iters, relres, status = op.solve(B, 0.5)                      # the call itself returns 0 (asserted in Op.solve)
        assert status[0] == 2 and np.isfinite(X[:, 0]).all()
        assert (status[1], iters[1]) == (0, 0) and np.all(X[:, 1] == 0.0)


@pytest.mark.parametrize("make", ("create", "decay"))
def test_a_column_of_a_solve_is_the_one_column_solve_bit_for_bit(mx, make):
    snps, indiv = 777, 515
    last = _window(snps, "w=256")
    if make == "create":
        op, shift = _create(mx, _case(snps, indiv, "plain"), "plain", snps, indiv, last, 0), 0.5
    else:
        op, shift = _from_rows(mx, last, opr.decay_rows(last)), 1.5
    with op:
        W = opr.windowed(ar.dense(op.rows(), last), last)
        B = _rhs(snps, W)
        X, iters, relres, status = op.solve(B, shift)
        assert np.all(status == 0) and len(set(iters.tolist())) >= 3, iters      # the columns stop at different iterations
        Xd, itd, reld, std = op.solve(B, shift, device=True)
        assert np.array_equal(_bits(Xd), _bits(X)) and np.array_equal(itd, iters) and np.array_equal(_bits(reld), _bits(relres)) and np.array_equal(std, status)
        for c in range(5):
            x1, it1, rel1, st1 = op.solve(B[:, c: c + 1], shift)
            assert np.array_equal(_bits(x1[:, 0]), _bits(X[:, c])), c
            assert (it1[0], st1[0]) == (iters[c], status[c]) and _bits(rel1)[0] == _bits(relres)[c], c
        assert np.array_equal(_bits(op.solve(B, shift)[0]), _bits(X)), "run to run"


# ----------------------------------------------------------------------------------------------------------------------------------- 6. errors
def test_bad_arguments_return_one_and_leave_everything_untouched(mx):
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    snps, indiv, n = 300, 40, 3
    prob = make_problem(snps, indiv, 1, seed=9)
    X, f = prob["plink"], prob["f"]
    good = ref.fixed_last(snps, 10)
    decreasing, beyond = good.copy(), good.copy()
    decreasing[7] = 30
    beyond[-1] = snps
    bad = (1, 1)

    # creation: *op is left NULL
    def create(plink=X, ns=snps, ni=indiv, last=good, kind=0, freq=f, pairwise=False, with_op=True):
        h = ctypes.c_void_p(0xdead)
        ref_h = ctypes.byref(h) if with_op else None
        if pairwise:
            rc = L.mxa_ld_op_create_pairwise(p(plink), ns, ni, p(last), kind, ref_h)
        else:
            rc = L.mxa_ld_op_create(p(plink), ns, ni, p(last), kind, 1, p(freq), ref_h)
        return rc, L.mxa_last_error(), (h.value if with_op else None)

    for pw in (False, True):
        for kw in (dict(plink=None), dict(ns=0), dict(ni=0), dict(last=None), dict(last=decreasing), dict(last=beyond), dict(kind=2), dict(kind=-1)):
            assert create(pairwise=pw, **kw) == (1, 1, None), (pw, kw)
        assert create(pairwise=pw, with_op=False)[:2] == bad
    assert create(freq=None) == (1, 1, None)
    rows = np.ones(int(ref.rowptr_of(good)[-1]))

    def from_rows(ns=snps, last=good, r=rows):
        h = ctypes.c_void_p(0xdead)
        return L.mxa_ld_op_from_rows(ns, p(last), p(r), ctypes.byref(h)), L.mxa_last_error(), h.value

    for kw in (dict(ns=0), dict(last=None), dict(r=None), dict(last=decreasing), dict(last=beyond)):
        assert from_rows(**kw) == (1, 1, None), kw
    assert (L.mxa_ld_op_from_rows(snps, p(good), p(rows), None), L.mxa_last_error()) == bad

    with _create(mx, dict(X=X, f=f), "plain", snps, indiv, good, 0) as op:
        Xp = np.ones((n, snps))
        nan, inf = float("nan"), float("inf")

        def apply(h=op.h, shift=0.5, x=Xp, ldx=snps, cols=n, ldy=snps, y="own"):
            Y = np.full((n + 1) * snps, SENTINEL)
            rc = L.mxa_ld_op_apply(h, shift, p(x), ldx, cols, p(Y) if isinstance(y, str) else y, ldy)
            return rc, L.mxa_last_error(), bool(np.all(Y == SENTINEL))

        for kw in (dict(h=None), dict(x=None), dict(y=None), dict(cols=0), dict(cols=-2), dict(ldx=snps - 1), dict(ldy=snps - 1), dict(shift=nan), dict(shift=inf),
                   dict(shift=-inf), dict(h=ctypes.c_void_p(Xp.ctypes.data))):
            assert apply(**kw) == (1, 1, True), kw
        # overlap between pointers of the same kind: Y inside X, and Y = X
        buf = np.ones((2 * n + 1) * snps)
        before = buf.copy()
        for off in (0, snps, (n - 1) * snps + snps - 1):
            rc = L.mxa_ld_op_apply(op.h, 0.0, p(buf), snps, n, ctypes.c_void_p(buf.ctypes.data + 8 * off), snps)
            assert (rc, L.mxa_last_error()) == bad and np.array_equal(buf, before), off
        assert L.mxa_ld_op_apply(op.h, 0.0, p(buf), snps, n, ctypes.c_void_p(buf.ctypes.data + 8 * n * snps), snps) == 0      # adjacent, not overlapping
        import torch
        dbuf = torch.ones((2 * n + 1) * snps, dtype=torch.float64, device="cuda")
        rc = L.mxa_ld_op_apply(op.h, 0.0, p(dbuf), snps, n, ctypes.c_void_p(dbuf.data_ptr() + 8 * snps), snps)
        assert (rc, L.mxa_last_error()) == bad and bool((dbuf == 1.0).all())
        assert apply() == (0, 0, False)

        def solve(h=op.h, shift=0.5, b=Xp, ldb=snps, cols=n, ldx=snps, x="own", tol=1e-8, max_iter=10):
            Xs = np.full((n + 1) * snps, SENTINEL)
            it, rel, st = np.full(n, -7, np.int32), np.full(n, SENTINEL), np.full(n, -7, np.int32)
            rc = L.mxa_ld_op_solve(h, shift, p(b), ldb, cols, p(Xs) if isinstance(x, str) else x, ldx, tol, max_iter, p(it), p(rel), p(st))
            return rc, L.mxa_last_error(), bool(np.all(Xs == SENTINEL) and np.all(it == -7) and np.all(rel == SENTINEL) and np.all(st == -7))

        for kw in (dict(h=None), dict(b=None), dict(x=None), dict(cols=0), dict(ldb=snps - 1), dict(ldx=snps - 1), dict(shift=nan), dict(shift=inf), dict(tol=0.0),
                   dict(tol=1.0), dict(tol=-1e-3), dict(tol=nan), dict(max_iter=-1), dict(h=ctypes.c_void_p(Xp.ctypes.data))):
            assert solve(**kw) == (1, 1, True), kw
        rc = L.mxa_ld_op_solve(op.h, 0.5, p(buf), snps, n, ctypes.c_void_p(buf.ctypes.data + 8 * snps), snps, 1e-8, 10, None, None, None)
        assert (rc, L.mxa_last_error()) == bad
        assert solve() == (0, 0, False)
        assert solve(max_iter=0)[:2] == (0, 0)
        assert (L.mxa_ld_op_rows(op.h, None), L.mxa_last_error()) == bad
        assert (L.mxa_ld_op_rows(None, p(rows)), L.mxa_last_error()) == bad
        stale = ctypes.c_void_p(op.h.value)
    # free twice, NULL, use after free
    assert op.h.value is None
    L.mxa_ld_op_free(ctypes.byref(op.h))
    L.mxa_ld_op_free(None)
    Y = np.full(n * snps, SENTINEL)
    assert (L.mxa_ld_op_apply(stale, 0.0, p(Xp), snps, n, p(Y), snps), L.mxa_last_error()) == bad and np.all(Y == SENTINEL)
    assert (L.mxa_ld_op_rows(stale, p(rows)), L.mxa_last_error()) == bad
    L.mxa_ld_op_free(ctypes.byref(stale))                                # a handle that is no longer live: a no-op that clears the pointer
    assert stale.value is None


# ------------------------------------------------------------------------------------------------------------------------------ 7. Python class
def test_python_class_end_to_end(mx):
    import torch
    snps, indiv = 777, 515
    case = _case(snps, indiv, "plain")
    cp = mx.crossproduct
    X, f = case["X"], case["f"]
    Xm = _x(snps, n=3)
    kw = dict(is_plink_format=True, allele_freq=f)
    last = ref.fixed_last(snps, 40)
    with cp.LdOperator.create(X, snps, indiv, window=40, kind="r", **kw) as op:
        assert (op.entries, op.nbytes) == cp.ld_op_bytes(last) and op.entries == int(ref.rowptr_of(last)[-1])
        rows = op.rows()
        assert isinstance(rows, np.ndarray) and np.array_equal(rows, cp.ld_window_rows(X, snps, indiv, last, kind="r", **kw))
        Y = op.apply(Xm, shift=0.25)
        assert isinstance(Y, np.ndarray) and Y.shape == (snps, 3)
        with _create(mx, case, "plain", snps, indiv, last, 0) as raw:
            assert np.array_equal(Y, raw.apply(Xm, 0.25))
        y1 = op.apply(Xm[:, 1], shift=0.25)                              # 1-D X: one column
        assert y1.shape == (snps,) and np.array_equal(y1, Y[:, 1])
        out = np.zeros((snps, 3), order="F")
        assert op.apply(Xm, shift=0.25, out=out) is out and np.array_equal(out, Y)
        dev = torch.device("cuda", 0)
        Yd = op.apply(torch.from_numpy(Xm).to(dev), shift=0.25)
        assert Yd.is_cuda and tuple(Yd.shape) == (snps, 3) and np.array_equal(Yd.cpu().numpy(), Y)
        assert op.rows(like=Yd).is_cuda
        Xs, iters, relres, status = op.solve(Xm, 2.0, tol=TOL)
        assert Xs.shape == (snps, 3) and np.all(status == 0) and np.all(relres <= TOL) and iters.dtype == np.int32
        W = opr.windowed(ar.dense(rows, last), last)
        assert np.all(opr.true_relres(W, 2.0, Xs, Xm) <= 2 * TOL)
        Xt, it_t, _, _ = op.solve(torch.from_numpy(Xm).to(dev), 2.0, tol=TOL)
        assert Xt.is_cuda and np.array_equal(Xt.cpu().numpy(), Xs) and np.array_equal(it_t, iters)
        xs1 = op.solve(Xm[:, 2], 2.0, tol=TOL)[0]
        assert xs1.shape == (snps,) and np.array_equal(xs1, Xs[:, 2])
        with cp.LdOperator.from_rows(last, rows) as twin:
            assert np.array_equal(twin.apply(Xm, shift=0.25), Y)
        with pytest.raises(ValueError, match="X needs to be"):
            op.apply(np.ones((snps + 1, 2)))
        with pytest.raises(ValueError, match="tol needs to be"):
            op.solve(Xm, 1.0, tol=1.0)
    with pytest.raises(RuntimeError, match="has been freed"):
        op.apply(Xm)
    op.free()
    casep = _case(snps, indiv, "pairwise-missing")
    with cp.LdOperator.create(casep["X"], snps, indiv, last=last, kind="r2", pairwise=True) as opp:
        assert np.array_equal(opp.rows(), cp.ld_window_rows_pairwise(casep["X"], snps, indiv, last, kind="r2"))
