"""Solver twin at its edges, checked exactly (fixtures: _solve_exact.py).

Dense: potrs_solve_gpu on L L^T of the exact family must return X_true bit for bit, at n and nrhs chosen against the schedule of
mxa_solve.hip (64-column blocks, 512-column panels, the L(p) / B(p) lookahead split) and the 128 x 128 tiles of k_dgemm; it reads only the
lower triangle; host and device pointers give the same bits; a failing minor is reported with its global index and X stays unwritten.
General SPD matrices: normwise backward error below n 2^-53 with the residual in extended precision.
Sparse: dcsrtrsv_solve_gpu on the exact triangular family must return X_true bit for bit across row lengths (up to 699 off-diagonal
entries), partial last workgroups, ncol around the 8-column pass and every transA; sparse2gpu's input errors name the row."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.linalg
import scipy.linalg.lapack
import scipy.sparse

from _solve_exact import exact_factor, exact_inverse_factor, exact_logdet, exact_rhs, exact_spd, exact_triangular

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


@functools.lru_cache(maxsize=4)
def _spd(n):
    M, L, d = exact_spd(n, seed=n)
    M.setflags(write=False)
    return M, L, d


def _logdet_tol(n, ld):
    # k_logdet: per thread a serial sum of n / 1024 terms, then a 10-level tree; plus one rounding of log on each side
    return (n / 1024 + 13) * U * max(ld, 1.0)


def _potrs(mx, A, n, B, nrhs, X, logdet):
    """potrs_solve_gpu on any mix of numpy arrays and torch tensors (column-major); returns (status, message)"""
    L = mx.lib.check_library_handle()
    st = ctypes.c_int(-1)
    p = mx.lib.ptr
    L.potrs_solve_gpu(p(A), n, p(B), nrhs, p(X), p(logdet), 0, ctypes.byref(st))
    return st.value, mx.lib.last_error()[1]


DENSE_N = [1, 2, 63, 64, 65, 128, 129, 511, 512, 513, 1024, 1025, 1153, 1600, 2049, 3001, 4096]
DENSE_CASES = [(n, r) for n in DENSE_N for r in (1, 17)] + [(n, r) for n in (65, 1153, 2049) for r in (128, 129, 257)]


@pytest.mark.parametrize("n,nrhs", DENSE_CASES)
def test_dense_exact_family(mx, n, nrhs):
    M, _, d = _spd(n)
    X_true, B = exact_rhs(M, nrhs, seed=n + nrhs)
    X, ld = mx.solve.dense_solve(M, B)
    assert np.array_equal(X, X_true), f"{np.count_nonzero(X != X_true)} entries differ, max |dX| = {np.abs(X - X_true).max():.3g}"
    ref = exact_logdet(d)
    assert abs(ld - ref) <= _logdet_tol(n, ref), (ld, ref)


def test_dense_exact_inverse(mx):
    n = 700
    M, L, d = _spd(n)
    Li = exact_inverse_factor(L, d)
    Minv = Li.T @ Li                                  # exact: dyadic partial sums
    X = mx.solve.dense_solve(M, np.eye(n), calc_logdet=False)
    assert np.array_equal(X, Minv)


@pytest.mark.parametrize("n", [1153, 2049])
def test_dense_reads_only_the_lower_triangle(mx, n):
    M, _, _ = _spd(n)
    X_true, B = exact_rhs(M, 17, seed=3)
    Mu = np.array(M, order="F")
    Mu[np.triu_indices(n, 1)] = np.nan
    X0, ld0 = mx.solve.dense_solve(M, B)
    X1, ld1 = mx.solve.dense_solve(Mu, B)
    assert np.array_equal(X0, X_true)
    assert np.array_equal(X1, X0) and ld1 == ld0


@pytest.mark.parametrize("n,nrhs", [(1153, 17), (2049, 129)])
def test_dense_device_and_host_pointers_agree(mx, n, nrhs):
    import torch
    M, _, d = _spd(n)
    X_true, B = exact_rhs(M, nrhs, seed=5)
    Mf, Bf = np.asfortranarray(M), np.asfortranarray(B)
    runs = []
    for _ in range(2):
        X = np.full((n, nrhs), -7.0, order="F")
        ld = np.zeros(1)
        assert _potrs(mx, Mf, n, Bf, nrhs, X, ld) == (0, "")
        runs.append((X, ld[0]))
    # device: column-major n x k is a row-major k x n tensor
    dA = torch.from_numpy(np.ascontiguousarray(Mf.T)).cuda()
    dB = torch.from_numpy(np.ascontiguousarray(Bf.T)).cuda()
    dX = torch.full((nrhs, n), -7.0, dtype=torch.float64, device="cuda")
    dld = torch.zeros(1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert _potrs(mx, dA, n, dB, nrhs, dX, dld) == (0, "")
    torch.cuda.synchronize()
    Xd, ldd = dX.cpu().numpy().T, float(dld.cpu()[0])
    assert np.array_equal(runs[0][0], X_true)
    assert np.array_equal(runs[1][0], runs[0][0]) and runs[1][1] == runs[0][1]      # same input, same bits: no race in the lookahead
    assert np.array_equal(Xd, runs[0][0]) and ldd == runs[0][1]
    assert abs(ldd - exact_logdet(d)) <= _logdet_tol(n, exact_logdet(d))


@pytest.mark.parametrize("how", ["negative_pivot", "nan"])
@pytest.mark.parametrize("j", [1, 64, 65, 513, 1100, 1153])
def test_dense_not_positive_definite_reports_the_minor(mx, j, how):
    n = 1153
    M, _, d = _spd(n)
    Mb = np.array(M, order="F")
    Mb[j - 1, j - 1] -= d[j - 1] ** 2 + 1.0               # the j-th pivot becomes exactly -1; pivots 1 .. j-1 are unchanged
    assert scipy.linalg.lapack.dpotrf(Mb, lower=1)[1] == j
    if how == "nan":
        Mb[j - 1, j - 1] = np.nan                           # (the CPU LAPACK here does not test its pivots for NaN; LAPACK's dpotf2 does)
    X_true, B = exact_rhs(M, 3, seed=j)
    Bf = np.asfortranarray(B)
    X = np.full((n, 3), 12345.0, order="F")
    ld = np.full(1, 54321.0)
    st, msg = _potrs(mx, Mb, n, Bf, 3, X, ld)
    assert st == 1
    assert msg.endswith(f"minor {j}"), msg
    assert np.all(X == 12345.0) and ld[0] == 54321.0


def test_dense_beyond_2_pow_31_elements(mx):
    """n = 46 400: A holds 2.15e9 elements (17.2 GB); M is assembled in Fortran order from a sparse L (only the lower triangle is written:
    the solver reads nothing else), so nothing of that size is copied."""
    import time
    n, nrhs = 46_400, 2
    Lsp, d = exact_factor(n, seed=7, per_row=4)
    Msp = (Lsp @ Lsp.T).tocoo()
    low = Msp.row >= Msp.col
    A = np.zeros((n, n), order="F")
    A[Msp.row[low], Msp.col[low]] = Msp.data[low]
    X_true = np.random.default_rng(8).integers(-4, 5, size=(n, nrhs)).astype(np.float64)
    B = np.asfortranarray(Msp.tocsr() @ X_true)
    X = np.zeros((n, nrhs), order="F")
    ld = np.zeros(1)
    t0 = time.perf_counter()
    st, msg = _potrs(mx, A, n, B, nrhs, X, ld)
    print(f"potrs_solve_gpu n = {n}: {time.perf_counter() - t0:.2f} s")
    del A
    assert st == 0, msg
    assert np.array_equal(X, X_true)
    assert abs(ld[0] - exact_logdet(d)) <= _logdet_tol(n, exact_logdet(d))


@functools.lru_cache(maxsize=2)
def _general(n):
    """M = G G^T / n with G n x n/2 (rank n/2: its smallest eigenvalue is 0) and its largest eigenvalue"""
    G = np.random.default_rng(n).standard_normal((n, n // 2))
    S = G @ G.T / n
    lmax = scipy.linalg.eigvalsh(S, subset_by_index=[n - 1, n - 1])[0]
    return S, lmax


@pytest.mark.parametrize("cond", [1e2, 1e6, 1e10])
@pytest.mark.parametrize("n,nrhs", [(1025, 1), (1025, 129), (2049, 1), (2049, 129)])
def test_dense_general_backward_error(mx, n, nrhs, cond):
    S, lmax = _general(n)
    M = S + (lmax / (cond - 1.0)) * np.eye(n)           # (lmax + delta) / delta = cond
    B = np.random.default_rng(n + nrhs).standard_normal((n, nrhs))
    X, ld = mx.solve.dense_solve(M, B)
    Ml, Xl, Bl = M.astype(np.longdouble), X.astype(np.longdouble), B.astype(np.longdouble)
    R = Bl - Ml @ Xl
    inf = lambda Z: np.abs(Z).sum(axis=1).max()
    eta = float(inf(R) / (inf(Ml) * inf(Xl) + inf(Bl)))
    print(f"n = {n} nrhs = {nrhs} cond = {cond:.0e}: backward error {eta:.3g} ({eta / U:.2f} u)")
    assert eta <= n * U, eta
    if cond == 1e2:
        sign, ld_ref = np.linalg.slogdet(M)
        assert sign == 1.0 and abs(ld - ld_ref) <= 1e-12 * abs(ld_ref), (ld, ld_ref)


# ------------------------------------------------------------------------------------------------ sparse

def _coo(T):
    c = T.tocoo()
    return c.data.copy(), (c.row + 1).astype(np.int64), (c.col + 1).astype(np.int64)


SPARSE_NCOL = [1, 7, 8, 9, 16, 17, 33]
SPARSE_CASES = [(m, s) for m in (1, 2, 3, 5, 4097, 10_001) for s in ("random", "band")] + [(700, "full")]


@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("m,structure", SPARSE_CASES)
def test_sparse_exact_family(mx, m, structure, lower):
    sv = mx.solve
    T = exact_triangular(m, seed=m + 7 * lower, structure=structure, lower=lower)
    V, I, J = _coo(T)
    Tt = T.T.tocsr()
    for ncol in SPARSE_NCOL:
        X_true = np.random.default_rng(ncol).integers(-8, 9, size=(m, ncol)).astype(np.float64)
        BN, BT = T @ X_true, Tt @ X_true                  # exact: integers
        obj = sv.sparse_init(V, I, J, len(V), m, ncol, lower)
        try:
            for trans in "NnTtf":
                X = sv.sparse_solve(obj, trans, BN if trans in "Nn" else BT, m)
                assert np.array_equal(X, X_true), (ncol, trans, np.count_nonzero(X != X_true))
        finally:
            sv.sparse_free(obj)


def test_sparse_chain_many_right_hand_sides(mx):
    """The bidiagonal chain of test_solve_gpu.py with 20 right-hand sides (three 8-column passes per row), one constant per column"""
    sv = mx.solve
    n, ncol = 100_000, 20
    I = np.concatenate([np.arange(1, n + 1), np.arange(2, n + 1)]).astype(np.int64)
    J = np.concatenate([np.arange(1, n + 1), np.arange(1, n)]).astype(np.int64)
    V = np.concatenate([np.full(n, 2.0), np.full(n - 1, -1.0)])
    c = np.arange(1.0, ncol + 1.0) * 0.37
    B = np.tile(c, (n, 1))
    obj = sv.sparse_init(V, I, J, len(V), n, ncol, True)
    try:
        X = sv.sparse_solve(obj, "n", B, n)              # x_i = (c + x_{i-1}) / 2
        Xt = sv.sparse_solve(obj, "t", B, n)             # x_i = (c + x_{i+1}) / 2
    finally:
        sv.sparse_free(obj)
    ref = np.empty((n, ncol))
    acc = np.zeros(ncol)
    for i in range(n):
        acc = (c + acc) / 2.0
        ref[i] = acc
    assert np.array_equal(X, ref)
    assert np.array_equal(Xt, ref[::-1])


def test_sparse_device_and_host_pointers_agree(mx):
    import torch
    sv = mx.solve
    L = mx.lib.check_library_handle()
    m, ncol = 4097, 17
    T = exact_triangular(m, seed=11, structure="random", lower=False)
    V, I, J = _coo(T)
    X_true = np.random.default_rng(12).integers(-8, 9, size=(m, ncol)).astype(np.float64)
    obj = sv.sparse_init(V, I, J, len(V), m, ncol, False)
    try:
        for trans, Top in (("n", T), ("t", T.T.tocsr())):
            B = np.asfortranarray(Top @ X_true)
            Xh = sv.sparse_solve(obj, trans, B, m)
            dB = torch.from_numpy(np.ascontiguousarray(B.T)).cuda()
            dX = torch.full((ncol, m), -3.0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            st = ctypes.c_int(-1)
            L.dcsrtrsv_solve_gpu(obj, trans.encode(), mx.lib.ptr(dB), ncol, mx.lib.ptr(dX), ctypes.byref(st))
            torch.cuda.synchronize()
            assert st.value == 0, mx.lib.last_error()[1]
            assert np.array_equal(Xh, X_true)
            assert np.array_equal(dX.cpu().numpy().T, Xh)
    finally:
        sv.sparse_free(obj)


def _bad_inputs(lower):
    """one-based COO of a 6 x 6 triangular matrix with a full diagonal and one entry per row off it; then variants with one defect at row 4"""
    m = 6
    I = list(range(1, m + 1)) + (list(range(2, m + 1)) if lower else list(range(1, m)))
    J = list(range(1, m + 1)) + (list(range(1, m)) if lower else list(range(2, m + 1)))
    V = [2.0] * m + [1.0] * (m - 1)
    cases = {}
    Vz = list(V); Vz[3] = 0.0
    cases["zero_diagonal"] = (Vz, I, J, r"row 4 has no non-zero diagonal")
    cases["missing_diagonal"] = (V[:3] + V[4:], I[:3] + I[4:], J[:3] + J[4:], r"row 4 has no non-zero diagonal")
    cases["duplicate_diagonal"] = (V + [3.0], I + [4], J + [4], r"duplicate diagonal entry in row 4")
    cases["index_zero"] = (V + [1.0], I + [0], J + [1], r"index \(0, 1\) outside 1\.\.6")
    cases["index_m_plus_1"] = (V + [1.0], I + [4], J + [7], r"index \(4, 7\) outside 1\.\.6")
    return m, cases


@pytest.mark.parametrize("case", ["zero_diagonal", "missing_diagonal", "duplicate_diagonal", "index_zero", "index_m_plus_1"])
@pytest.mark.parametrize("lower", [True, False])
def test_sparse_init_errors_name_the_row(mx, case, lower):
    import re
    L = mx.lib.check_library_handle()
    m, cases = _bad_inputs(lower)
    V, I, J, pattern = cases[case]
    V, I, J = np.array(V), np.array(I, dtype=np.int64), np.array(J, dtype=np.int64)
    obj = ctypes.c_void_p(12345)
    st = ctypes.c_int(-1)
    L.sparse2gpu(mx.lib.ptr(V), mx.lib.ptr(I), mx.lib.ptr(J), len(V), m, 1, int(lower), ctypes.byref(obj), ctypes.byref(st))
    msg = mx.lib.last_error()[1]
    assert st.value == 1
    assert obj.value is None
    assert re.search(pattern, msg), msg
