"""References of the LD operator tests (mxa_ld_op_*): plain numpy, nothing of the library is imported.

    dyadic_rows(last, seed)        upper ragged rows with diagonal 1 and off-diagonals in {+-k / 8, k = 0 .. 8}: with small integer X and shift in {0, 0.5, -2}
                                   every product and every partial sum of the apply is an integer multiple of 1 / 8 far below 2^53, i.e. exact in any order
    decay_rows(last, seed)         T(d) = +-2^-min(d, 10), diagonal 1: the off-diagonal part has spectral norm below 2 + 2 sqrt(snps) 2^-10 < 2.5 for the
                                   sizes used here (a geometric band of norm < 2 plus a random-sign matrix of entries 2^-10), so T + 1.5 I is positive definite
    windowed(T, last)              T inside the window, 0.0 outside (the matrix the operator applies)
    apply_exact(W, X, shift)       W X + shift X in numpy float64 -- exact for the dyadic family, where it is compared bit for bit
    cg(W, shift, b, tol, max_iter) the conjugate-gradient recurrence of mxa_ld_op_solve on one column in numpy float64: (x, iters, relres, status)
    true_relres(W, shift, X, B)    |B - (W + shift I) X|_2 / |B|_2 per column in long double
"""
import numpy as np

import _ld_ref as ref

U = 2.0 ** -53
LD = np.longdouble


def _signs(total, rng):
    return np.where(rng.random(total) < 0.5, -1.0, 1.0)


def dyadic_rows(last, seed=11):
    ii, jj = ref.pairs(last)
    rng = np.random.default_rng([len(last), seed])
    v = _signs(len(ii), rng) * rng.integers(0, 9, len(ii)) / 8.0
    v[ii == jj] = 1.0
    return v


def decay_rows(last, seed=13):
    ii, jj = ref.pairs(last)
    rng = np.random.default_rng([len(last), seed])
    v = _signs(len(ii), rng) * 2.0 ** -np.minimum(jj - ii, 10).astype(np.float64)
    v[ii == jj] = 1.0
    return v


def inside(last):
    n = len(last)
    first = ref.first_of(last)
    j = np.arange(n)
    return (j[None, :] >= first[:, None]) & (j[None, :] <= np.asarray(last)[:, None])


def windowed(T, last):
    return np.where(inside(last), T, 0.0)


def apply_exact(W, X, shift):
    return W @ X + shift * X


def cg(W, shift, b, tol, max_iter):
    """the recurrence of mxa_ld_op_solve, one column: x = 0, r = p = b; the test |r| / |b| <= tol before the first iteration and after every update; breakdown
    (status 2) when p.Ap is not > 0; status 1 when max_iter updates did not converge"""
    x = np.zeros_like(b)
    r, p = b.copy(), b.copy()
    rr = bb = float(r @ r)
    if bb == 0.0:
        return x, 0, 0.0, 0
    it, rel = 0, 1.0
    while True:
        if it == max_iter:
            return x, it, rel, 1
        Ap = W @ p + shift * p
        pAp = float(p @ Ap)
        if not pAp > 0.0:
            return x, it, rel, 2
        alpha = rr / pAp
        x = x + alpha * p
        r = r - alpha * Ap
        rrn = float(r @ r)
        it += 1
        rel = float(np.sqrt(rrn) / np.sqrt(bb))
        if rel <= tol:
            return x, it, rel, 0
        p = r + (rrn / rr) * p
        rr = rrn


def true_relres(W, shift, X, B):
    Wl = W.astype(LD)
    R = B.astype(LD) - (Wl @ X.astype(LD) + LD(shift) * X.astype(LD))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (np.sqrt((R * R).sum(axis=0)) / np.sqrt((B.astype(LD) ** 2).sum(axis=0))).astype(np.float64)
