"""References of the score-test tests (mxa_assoc_logistic_null / mxa_assoc_score).  numpy, fractions and math only; nothing of the library is imported.

score_family    inputs R, Wt, H on which every sum the definition names is exact in fp64 in any order
chain_score     the documented chain from those exact sums, every operation rounded once: the GPU result bit for bit
bounded_score   U, V, z on arbitrary real data in np.longdouble from the same R, Wt, H, with a first-order forward bound per element
textbook_chi2   U^2 / V with an explicit (C^T W C)^-1 in np.longdouble, from the null design itself: what H stands for
newton_ld       the logistic null model by Newton's iteration in np.longdouble, run to a fixed point
binary_case     genotypes with 5 % missing calls, raw covariates and 0 / 1 traits drawn from a logistic model with a small genetic effect
"""
import numpy as np

from _assoc_ref import LD, U, div, exact_family, fma, genotypes, pack, same_bits, sqrt, walsh  # noqa: F401

P_OF_M = {16: 2, 64: 3, 256: 4, 1024: 5, 16384: 7, 65536: 8}


def score_family(indiv, n, kh, seed):
    """(R (indiv, n), Wt (indiv, n), H (indiv, n kh)), Fortran-ordered float64, indiv = m + 3 with m = 4^p.  R: exact_family(indiv, n, 0, seed).  Wt: entries from
    {1, 2, 3, 4} / 16.  H: Walsh functions times 2^-(p + 2) on the first m individuals, entries from {-2 .. 2} / 16 on the last three.  Every entry is a small
    multiple of a power of two, so every sum of entries over any set of individuals, times 0, 1 or 2, is exact in fp64 in any order."""
    m = indiv - 3
    p = P_OF_M[m]
    rng = np.random.default_rng([seed, indiv, n, kh, 77])
    R = exact_family(indiv, n, 0, seed)[0]
    Wt = np.asfortranarray(rng.integers(1, 5, (indiv, n)) / 16.0)
    H = np.zeros((indiv, n * kh), order="F")
    for j in range(n * kh):
        H[:m, j] = walsh(m, int(rng.integers(1, m))) * 2.0 ** -(p + 2)
        H[m:, j] = rng.integers(-2, 3, 3) / 16.0
    return R, Wt, H


def score_sums(codes, R, Wt, H, dtype=np.float64):
    """N, Sz (ints), D = Z^T B, M = (missing)^T B for B = [R | Wt | H], E = (code 11)^T Wt"""
    codes = np.asarray(codes)
    B = np.concatenate([R, Wt, H], axis=1).astype(dtype)
    z = np.where(codes < 0, 0, codes).astype(dtype)
    miss = (codes < 0).astype(dtype)
    N = (codes >= 0).sum(1).astype(np.int64)
    Sz = (codes == 1).sum(1).astype(np.int64) + 2 * (codes == 2).sum(1).astype(np.int64)
    return N, Sz, z @ B, miss @ B, (codes == 2).astype(dtype) @ Wt.astype(dtype)


def chain_score(codes, R, Wt, H):
    """score, var, z (snps, n) and nobs by the documented chain from exact sums (the exact family)"""
    n = R.shape[1]
    kh = H.shape[1] // n if n else 0
    N, Sz, D, M, E = score_sums(codes, R, Wt, H)
    snps = np.asarray(codes).shape[0]
    score, var, z = (np.zeros((snps, n)) for _ in range(3))
    for s in range(snps):
        mu = div(float(Sz[s]), float(N[s]))
        m2 = float(np.float64(mu) * np.float64(mu))
        for c in range(n):
            u = fma(mu, M[s, c], D[s, c])
            s2 = fma(2.0, E[s, c], D[s, n + c])
            sxx = fma(m2, M[s, n + c], s2)
            for j in range(kh):
                b = 2 * n + c * kh + j
                a = fma(mu, M[s, b], D[s, b])
                sxx = fma(-a, a, sxx)
            score[s, c], var[s, c], z[s, c] = u, sxx, div(u, sqrt(sxx))
    return score, var, z, N.astype(np.int32)


def bounded_score(codes, R, Wt, H):
    """(U, V, z) in np.longdouble, (dU, dV, dz) first-order forward bounds per element, and the positive part sww = sum w x^2 of V per element.  Every inner
    product carries gamma sum |a_i| |b_i| with gamma = (indiv + 2 kh + 16) 2^-53 (any summation order; the model of tests/_assoc_ref.py::bounded); the chain
    propagates by the triangle inequality."""
    codes = np.asarray(codes)
    indiv, n = R.shape
    kh = H.shape[1] // n
    gam = LD((indiv + 2 * kh + 16) * U)
    N, Sz, D, M, E = score_sums(codes, R, Wt, H, LD)
    _, _, aD, aM, _ = score_sums(codes, np.abs(R), np.abs(Wt), np.abs(H), LD)
    dD, dM, dE = gam * aD, gam * aM, gam * E
    with np.errstate(all="ignore"):
        mu = (Sz.astype(LD) / N.astype(LD))[:, None]
        Dr, Mr, Dw, Mw = D[:, :n], M[:, :n], D[:, n:2 * n], M[:, n:2 * n]
        Uv = mu * Mr + Dr
        dU = dD[:, :n] + mu * dM[:, :n] + gam * (aD[:, :n] + mu * aM[:, :n])
        sww = Dw + 2 * E + mu * mu * Mw
        dV = dD[:, n:2 * n] + 2 * dE + mu * mu * dM[:, n:2 * n] + 3 * gam * sww
        V = sww.copy()
        for c in range(n):
            for j in range(kh):
                b = 2 * n + c * kh + j
                a = mu[:, 0] * M[:, b] + D[:, b]
                da = dD[:, b] + mu[:, 0] * dM[:, b] + gam * (aD[:, b] + mu[:, 0] * aM[:, b])
                V[:, c] -= a * a
                dV[:, c] += 2 * np.abs(a) * da + gam * (a * a)
        dV = dV + gam * np.abs(V)
        zv = Uv / np.sqrt(V)
        dz = dU / np.sqrt(V) + np.abs(zv) * (LD(0.5) * dV / V + gam)
    return (Uv, V, zv), (dU, dV, dz), sww


def imputed(codes):
    """x (snps, indiv) in np.longdouble: the allele counts, missing calls replaced by the SNP's mean over its called individuals"""
    codes = np.asarray(codes)
    x = np.where(codes < 0, 0, codes).astype(LD)
    mu = x.sum(1) / (codes >= 0).sum(1).astype(LD)
    return np.where(codes < 0, mu[:, None], x)


def textbook_chi2(codes, y, C, gamma):
    """U^2 / V per SNP for one trait from the null design itself, np.longdouble: p = expit(C gamma), U = x^T (y - p),
    V = x^T W x - x^T W C (C^T W C)^-1 C^T W x, W = diag(p (1 - p))"""
    C = np.asarray(C).astype(LD)
    p = 1 / (1 + np.exp(-(C @ np.asarray(gamma).astype(LD))))
    w = p * (1 - p)
    x = imputed(codes)
    Uv = x @ (np.asarray(y).astype(LD) - p)
    A = C.T @ (w[:, None] * C)
    G = x @ (w[:, None] * C)                                   # snps x (q + 1)
    Ainv = inverse_ld(A)
    V = (x * x) @ w - np.einsum("sa,ab,sb->s", G, Ainv, G)
    return Uv * Uv / V


def inverse_ld(A):
    """the inverse of a symmetric positive definite matrix in np.longdouble (Gauss-Jordan; numpy's linalg has no long double)"""
    k = A.shape[0]
    aug = np.concatenate([A.astype(LD), np.eye(k, dtype=LD)], axis=1)
    for i in range(k):
        aug[i] = aug[i] / aug[i, i]
        for r in range(k):
            if r != i:
                aug[r] = aug[r] - aug[r, i] * aug[i]
    return aug[:, k:]


def cholesky_ld(A):
    k = A.shape[0]
    L = np.zeros((k, k), LD)
    for a in range(k):
        for b in range(a + 1):
            s = A[a, b] - (L[a, :b] * L[b, :b]).sum()
            L[a, b] = np.sqrt(s) if a == b else s / L[b, b]
    return L


def newton_ld(y, C, max_iter=200):
    """(gamma, r, w, H) of the logistic null model in np.longdouble: plain Newton steps from the intercept logit(ybar) until the iterate no longer changes (a
    fixed point in long double), H = diag(w) C L^-T by forward substitution"""
    y = np.asarray(y).astype(LD)
    C = np.asarray(C).astype(LD)
    g = np.zeros(C.shape[1], LD)
    g[0] = np.log(y.mean() / (1 - y.mean()))
    for _ in range(max_iter):
        p = 1 / (1 + np.exp(-(C @ g)))
        w = p * (1 - p)
        A = C.T @ (w[:, None] * C)
        new = g + inverse_ld(A) @ (C.T @ (y - p))
        if np.abs(new - g).max() <= LD(2.0) ** -60 * max(1, np.abs(new).max()):
            g = new
            break
        g = new
    else:
        raise RuntimeError("the reference iteration did not reach a fixed point")
    p = 1 / (1 + np.exp(-(C @ g)))
    w = p * (1 - p)
    L = cholesky_ld(C.T @ (w[:, None] * C))
    X = np.zeros_like(C)                                        # row i: L^-1 c_i
    for a in range(C.shape[1]):
        X[:, a] = (C[:, a] - X[:, :a] @ L[a, :a]) / L[a, a]
    return g, y - p, w, w[:, None] * X


def binary_case(indiv, snps, n, q, seed, fraction=0.4):
    """codes (5 % missing, no edge patterns), Y (indiv, n) of 0 / 1 with about `fraction` cases, from a logistic model in the covariates and three SNPs with a
    small effect, W (indiv, q) raw covariates with offsets"""
    rng = np.random.default_rng([seed, indiv, snps, n, q, 3])
    codes = genotypes(snps, indiv, seed, missing=0.05, special=False)
    W = rng.standard_normal((indiv, q)) + 0.3 * rng.standard_normal((indiv, 1)) + rng.uniform(-2, 2, q)
    z = np.where(codes < 0, 0, codes).astype(np.float64)
    eta = (W - W.mean(0)) @ (0.3 * rng.standard_normal((q, n))) + 0.2 * ((z[rng.integers(0, snps, 3)].T - 0.6) @ rng.standard_normal((3, n)))
    eta = eta + np.log(fraction / (1 - fraction))
    Y = (rng.random((indiv, n)) < 1 / (1 + np.exp(-eta))).astype(np.float64)
    return codes, np.asfortranarray(Y), np.asfortranarray(W)
