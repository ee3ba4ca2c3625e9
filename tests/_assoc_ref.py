"""References of the association scan tests (mxa_assoc_basis / mxa_assoc_linear).  numpy, fractions and math only; nothing of the library is imported.

codes           genotypes as an int8 array (snps, indiv): 0, 1, 2 = the allele count, -1 = a missing call
pack(codes)     the PLINK rows: (snps, ceil(indiv / 4)) uint8, 00 -> 0, 01 -> missing, 10 -> 1, 11 -> 2, low fields first, padding fields zero
exact_family    inputs on which every sum the definition names is exact in fp64 in any order, and the residualization is exactly the identity
chain_exact     the documented chain from those exact sums, every operation rounded once: the GPU result bit for bit
bounded         the same statistics on arbitrary real data in np.longdouble, with a first-order forward bound per element
restate_float64 a plain float64 numpy restatement of the definition (any order of the individuals): what a correct implementation may return
"""
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def pack(codes):
    codes = np.asarray(codes)
    snps, indiv = codes.shape
    field = np.where(codes < 0, 1, np.where(codes == 0, 0, codes + 1)).astype(np.uint8)
    full = np.zeros((snps, (indiv + 3) // 4 * 4), np.uint8)
    full[:, :indiv] = field
    q = full.reshape(snps, -1, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)


def genotypes(snps, indiv, seed, missing=0.05, special=True):
    """random codes with `missing` missing calls; special, from 7 SNPs on: the first six rows are the edge patterns -- entirely missing, one called individual,
    monomorphic (with and without missing calls), a missing call in the last field of the row, no missing call at all.  With fewer SNPs every row is an
    ordinary one, so that a one-SNP case compares finite statistics."""
    rng = np.random.default_rng([seed, snps, indiv])
    f = rng.uniform(0.1, 0.5, snps)
    codes = rng.binomial(2, f[:, None], (snps, indiv)).astype(np.int8)
    if missing > 0:
        codes[rng.random((snps, indiv)) < missing] = -1
    if special and snps >= 7:
        pats = []
        pats.append(np.full(indiv, -1, np.int8))                                   # entirely missing: N = 0
        one = np.full(indiv, -1, np.int8); one[indiv // 2] = 1; pats.append(one)   # one called individual
        pats.append(np.full(indiv, 2, np.int8))                                    # monomorphic, all called
        mono = np.full(indiv, 1, np.int8); mono[::5] = -1; pats.append(mono)       # monomorphic on its called individuals
        last = rng.binomial(2, 0.3, indiv).astype(np.int8); last[-1] = -1; pats.append(last)   # a missing code in the last (partial) byte
        pats.append(rng.binomial(2, 0.4, indiv).astype(np.int8))                   # no missing code
        for r, p in enumerate(pats):
            codes[r] = p
    return codes


# ---- the exact family
def walsh(m, j):
    i = np.arange(m)
    bits = np.zeros(m, np.int64)
    x = i & j
    while np.any(x):
        bits += x & 1
        x >>= 1
    return 1.0 - 2.0 * (bits & 1)


def exact_family(indiv, n, k, seed):
    """(Y (indiv, n), Q (indiv, k)), Fortran-ordered float64, indiv = m + 3 with m = 2^(2p) in {16, 64, 256, 1024, 16384, 65536}.  Q: distinct non-constant Walsh
    functions times 2^-p on the first m individuals, zero on the last three (exactly orthonormal, exactly zero-sum).  Y: small-integer combinations (|coefficient| <= 4) of OTHER Walsh functions, and integers
    that sum to zero on the last three.  Needs n >= 1 and k + 1 <= 4^p - 1 (one function at least is left for Y)."""
    m = indiv - 3
    p = {16: 2, 64: 3, 256: 4, 1024: 5, 16384: 7, 65536: 8}[m]           # m = 4^p = 2^(2p): the scale 2^-p makes the columns unit vectors
    assert 0 <= k <= m - 2, (indiv, k)
    rng = np.random.default_rng([seed, indiv, n, k])
    order = rng.permutation(np.arange(1, m))
    Q = np.zeros((indiv, k), order="F")
    for q in range(k):
        Q[:m, q] = walsh(m, int(order[q])) * 2.0 ** -p
    rest = order[k:]
    Y = np.zeros((indiv, n), order="F")
    for c in range(n):
        for j in rng.choice(rest, size=min(3, len(rest)), replace=False):
            Y[:m, c] += float(rng.choice([-4, -3, -2, -1, 1, 2, 3, 4])) * walsh(m, int(j))
        a, b = rng.integers(-4, 5, 2)
        Y[m:, c] = (a, b, -a - b)
    return Y, Q


def fma(a, b, c):
    """a * b + c rounded once, IEEE signs of zero, non-finite operands as the hardware treats them"""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        return a * b + c            # an exact zero: a * b is exact then (it is zero, or it is -c), and the float expression has the IEEE sign
    return float(r)


def div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def sqrt(a):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(a)))


def sums(codes, B):
    """N, Sz, Szz (exact ints), D = Z^T B, M = (missing)^T B, T = 1^T B in float64 -- exact, in any order, on the exact family"""
    codes = np.asarray(codes)
    z = np.where(codes < 0, 0, codes).astype(np.float64)
    miss = (codes < 0).astype(np.float64)
    N = (codes >= 0).sum(1).astype(np.int64)
    c1, c2 = (codes == 1).sum(1).astype(np.int64), (codes == 2).sum(1).astype(np.int64)
    return N, c1 + 2 * c2, c1 + 4 * c2, z @ B, miss @ B, B.sum(0)


def chain_exact(codes, Y, Q):
    """beta, se, t (snps, n) by the documented chain from exact sums (the exact family: Y~ = Y)"""
    indiv, n = Y.shape
    k = Q.shape[1]
    B = np.concatenate([Y, Q], axis=1)
    N, Sz, Szz, D, M, T = sums(codes, B)
    syy = (Y * Y).sum(0)
    dof = float(indiv - k - 2)
    snps = codes.shape[0]
    beta, se, t = (np.zeros((snps, n)) for _ in range(3))
    for s in range(snps):
        dN = float(N[s])
        mu = div(float(Sz[s]), dN)
        v0 = div(float(int(N[s]) * int(Szz[s]) - int(Sz[s]) ** 2), dN)
        sxx = v0
        for q in range(k):
            g = fma(mu, M[s, n + q] - T[n + q], D[s, n + q])
            sxx = fma(-g, g, sxx)
        for c in range(n):
            g = fma(mu, M[s, c] - T[c], D[s, c])
            b = div(g, sxx)
            rss = fma(-b, g, syy[c])
            e = sqrt(div(div(rss, dof), sxx))
            beta[s, c], se[s, c], t[s, c] = b, e, div(b, e)
    return beta, se, t, N.astype(np.int32)


def same_bits(got, want):
    """NaNs in the same places, every other element bit for bit"""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


# ---- real data
def real_case(indiv, snps, n, k, seed):
    """codes (5 % missing, no edge patterns), Y (mean 100, correlated with the covariates, a small genetic effect), W (indiv, k) raw covariates"""
    rng = np.random.default_rng([seed, indiv, snps, n, k])
    codes = genotypes(snps, indiv, seed, missing=0.05, special=False)
    W = rng.standard_normal((indiv, k)) + 0.3 * rng.standard_normal((indiv, 1)) + rng.uniform(-5, 5, k)
    z = np.where(codes < 0, 0, codes).astype(np.float64)
    Y = 100.0 + W @ rng.standard_normal((k, n)) + rng.standard_normal((indiv, n)) + 0.2 * (z[rng.integers(0, snps, 3)].T @ rng.standard_normal((3, n)))
    return codes, np.asfortranarray(Y), np.asfortranarray(W)


def bounded(codes, Y, Q):
    """(beta, se, t) in np.longdouble, (bound_beta, bound_se, bound_t) first-order forward bounds per element, and sxx, v0 per SNP.  Every inner product of
    length m carries gamma sum |a_i| |b_i|, gamma = (indiv + 2 k + 16) 2^-53 (it holds for any summation order); the chain propagates by the triangle inequality."""
    codes = np.asarray(codes)
    indiv, n = Y.shape
    k = Q.shape[1]
    gam = LD((indiv + 2 * k + 16) * U)
    y = Y.astype(LD)
    q = Q.astype(LD)
    y = y - y.mean(0)
    for _ in range(2):
        y = y - q @ (q.T @ y)
    B = np.concatenate([y, q], axis=1)
    aB = np.abs(B)
    z = np.where(codes < 0, 0, codes).astype(LD)
    miss = (codes < 0).astype(LD)
    N = (codes >= 0).sum(1).astype(LD)
    c1, c2 = (codes == 1).sum(1).astype(LD), (codes == 2).sum(1).astype(LD)
    Sz, Szz = c1 + 2 * c2, c1 + 4 * c2
    D, M, T = z @ B, miss @ B, B.sum(0)
    dD, dM, dT = gam * (z @ aB), gam * (miss @ aB), gam * aB.sum(0)
    syy = (y * y).sum(0)
    dsyy = gam * syy
    mu = (Sz / N)[:, None]
    v0 = (N * Szz - Sz * Sz) / N
    g = mu * (M - T) + D
    dg = dD + mu * (dM + dT) + gam * (np.abs(D) + mu * np.abs(M - T))
    gq, dgq = g[:, n:], dg[:, n:]
    sxx = v0 - (gq * gq).sum(1)
    dsxx = (2 * np.abs(gq) * dgq).sum(1) + gam * (v0 + (gq * gq).sum(1))
    gc, dgc = g[:, :n], dg[:, :n]
    sx, dsx = sxx[:, None], dsxx[:, None]
    beta = gc / sx
    dbeta = (dgc + np.abs(beta) * dsx) / sx + gam * np.abs(beta)
    rss = syy - beta * gc
    drss = dsyy + np.abs(beta) * dgc + np.abs(gc) * dbeta + gam * (syy + np.abs(beta * gc))
    dof = LD(indiv - k - 2)
    se = np.sqrt(rss / dof / sx)
    dse = se * (LD(0.5) * (drss / rss + dsx / sx) + gam)
    t = beta / se
    dt = dbeta / se + np.abs(t) * dse / se + gam * np.abs(t)
    return (beta, se, t), (dbeta, dse, dt), sxx, v0


def within_bound(got, ref, bound, keep, factor=4.0):
    """|got - ref| <= factor * bound on the SNPs `keep`; returns (ok, the largest |got - ref| / bound there)"""
    err = np.abs(np.asarray(got).astype(LD) - ref)[keep]
    ratio = float((err / bound[keep]).max())
    return bool(np.all(err <= LD(factor) * bound[keep])), ratio


def restate_float64(codes, Y, Q, reverse=False):
    """the definition in plain float64 numpy, the individuals summed in the given or in reversed order"""
    codes = np.asarray(codes)
    if reverse:
        codes, Y, Q = codes[:, ::-1], Y[::-1], Q[::-1]
    codes, Y, Q = np.ascontiguousarray(codes), np.ascontiguousarray(Y), np.ascontiguousarray(Q)
    indiv, n = Y.shape
    k = Q.shape[1]
    y = Y - Y.sum(0) / indiv
    for _ in range(2):
        y = y - Q @ (Q.T @ y)
    B = np.concatenate([y, Q], axis=1)
    N, Sz, Szz, D, M, T = sums(codes, B)
    syy = (y * y).sum(0)
    mu = (Sz / N)[:, None]
    v0 = (N * Szz - Sz * Sz) / N
    g = mu * (M - T) + D
    sxx = (v0 - (g[:, n:] ** 2).sum(1))[:, None]
    beta = g[:, :n] / sxx
    rss = syy - beta * g[:, :n]
    se = np.sqrt(rss / (indiv - k - 2) / sxx)
    return beta, se, beta / se
