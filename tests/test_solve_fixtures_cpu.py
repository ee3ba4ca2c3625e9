"""The exact fixtures of the solver twin (_solve_exact.py) and the numpy restatement of its blocked Cholesky schedule, on the CPU: the family's
claims hold bit for bit, the unfaulted schedule returns X_true bit for bit, and each of three planted schedule faults breaks the exact check
at one of the shapes of test_solve_exact_gpu.py while it passes the 1e-10 residual of test_solve_gpu.py's exp(-|i-j|/n) matrix at the
shapes that test uses (n = 100, 1000, 4000): the old suite cannot see these faults, the new one does."""
import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

from _solve_exact import (blocked_cholesky_solve, exact_inverse_factor, exact_logdet, exact_rhs, exact_spd, exact_triangular)


@pytest.mark.parametrize("n", [1, 2, 63, 65, 129, 513, 1153])
def test_exact_family_claims(n):
    M, L, d = exact_spd(n, seed=n)
    N = np.tril(L, -1)
    assert set(np.unique(N)) <= {-1.0, 0.0, 1.0} and set(np.unique(d)) <= {1.0, 2.0}
    assert not np.any(N @ np.diag(1.0 / d) @ N)                              # N D^-1 N = 0
    Li = exact_inverse_factor(L, d)
    assert np.array_equal(Li @ L, np.eye(n)) and np.array_equal(L @ Li, np.eye(n))
    assert np.array_equal(np.linalg.cholesky(M), L)
    assert np.array_equal(M, M.T) and np.array_equal(M, np.round(M))
    Minv = Li.T @ Li
    assert np.array_equal(M @ Minv, np.eye(n))                               # M^-1 = L^-T L^-1, exactly
    sign, ld = np.linalg.slogdet(M)
    assert sign == 1.0 and abs(ld - exact_logdet(d)) <= 1e-12 * max(1.0, ld)


@pytest.mark.parametrize("n,nrhs", [(1, 1), (64, 17), (65, 129), (513, 17), (1025, 17), (1153, 3), (2049, 17)])
def test_unfaulted_schedule_is_exact(n, nrhs):
    M, L, d = exact_spd(n, seed=n)
    X_true, B = exact_rhs(M, nrhs, seed=n + 1)
    X, ld = blocked_cholesky_solve(M, B)
    assert np.array_equal(X, X_true)
    assert abs(ld - exact_logdet(d)) <= 8 * np.spacing(max(1.0, exact_logdet(d)))


def test_schedule_reads_only_the_lower_triangle():
    M, _, _ = exact_spd(600, seed=5)
    X_true, B = exact_rhs(M, 4, seed=6)
    Mu = M.copy()
    Mu[np.triu_indices(600, 1)] = np.nan
    assert np.array_equal(blocked_cholesky_solve(Mu, B)[0], X_true)


def _old_suite_passes(fault):
    """test_solve_gpu.py::test_dense_cholesky_solve_and_logdet's criterion at its own shapes"""
    for n, ncol in [(100, 1), (1000, 5), (4000, 20)]:
        idx = np.arange(n, dtype=np.float64)
        M = np.exp(-np.abs(idx[:, None] - idx[None, :]) / n) + 1e-3 * np.eye(n)
        B = np.random.default_rng(n).standard_normal((n, ncol)) + 5.0
        X, _ = blocked_cholesky_solve(M, B, fault)
        if not np.linalg.norm(M @ X - B) / np.linalg.norm(B) < 1e-10:
            return False
    return True


# fault -> the (n, nrhs) of test_solve_exact_gpu.py that must expose it
PLANTED = {
    "skip_far_small": [(1025, 17), (2049, 17)],    # far = 1 at n = 1025 (panel 0) and n = 2049 (panel 2)
    "skip_next_small": [(513, 17), (1025, 17)],    # one row trails the last full panel
    "rhs_first_tile": [(65, 129), (65, 257)],      # the second column tile of the solve products
}


@pytest.mark.parametrize("fault", sorted(PLANTED))
def test_planted_fault_escapes_the_old_suite_and_breaks_the_exact_check(fault):
    assert _old_suite_passes(fault)
    for n, nrhs in PLANTED[fault]:
        M, _, _ = exact_spd(n, seed=n)
        X_true, B = exact_rhs(M, nrhs, seed=n + 1)
        X, _ = blocked_cholesky_solve(M, B, fault)
        assert not np.array_equal(X, X_true), (fault, n, nrhs)


@pytest.mark.parametrize("structure,m", [("random", 4097), ("band", 1000), ("full", 300)])
@pytest.mark.parametrize("lower", [True, False])
def test_sparse_family_substitution_is_exact(structure, m, lower):
    T = exact_triangular(m, seed=m, structure=structure, lower=lower)
    Td = T.toarray()
    assert np.array_equal(np.tril(Td) if lower else np.triu(Td), Td)
    assert set(np.unique(np.diag(Td))) <= {-2.0, -1.0, -0.5, 0.5, 1.0, 2.0}
    X_true = np.random.default_rng(1).integers(-8, 9, size=(m, 3)).astype(np.float64)
    for op in (T, T.T.tocsr()):
        B = op @ X_true
        X = scipy.sparse.linalg.spsolve_triangular(op.tocsr(), B, lower=(op is T) == lower)
        assert np.array_equal(X, X_true)
    if structure == "band":
        assert np.diff(T.indptr).max() == 201
