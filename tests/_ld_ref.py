"""References of the windowed LD tests, from the definition: plain numpy, nothing of the library is imported, so mxa_ld is part of no reference.

Plain route (mxa_ld, mxa_ld_band, mxa_ld_scores, mxa_ld_window_rows, mxa_ld_window_scores)
    staged(X)      the values the library multiplies: raw 2-bit fields, or PLINK codes through the byte table 00 -> 0, 10 -> 1, 11 -> 2 with its quirk: a BYTE
                   that holds a missing pair (01) reads as four 3s, the padding fields of a row's last byte included.
    gram_exact(Z)  M = Z Z^T as exact integers: float64 BLAS over K chunks, every partial sum an integer below 2^53; a few rows are recomputed in int64.
    ld_ref(M,f,n)  c = M - 4 n f f^T, sigma = sqrt(diag c), r = c / (sigma sigma^T) in np.longdouble (64-bit mantissa), the caller's float64 f taken as given.

Element-wise bound of the library's map.  It computes, in float64 with u = 2^-53,
    c^_ij = fma(-4n, fl(f_i f_j), M_ij)        is_i = fl(1 / fl(sqrt(c^_ii)))        r^_ij = fl(c^_ij * fl(is_i * is_j)).
With A_ij = 4n |f_i f_j|:  fl(f_i f_j) = f_i f_j (1 + d0) moves c by at most u A_ij, the fma's one rounding by u |c_ij| (first order), so
    |c^_ij - c_ij| <= u (A_ij + |c_ij|),        c^_ii = c_ii (1 + eta_i),  |eta_i| <= eps_i = u (A_ii + c_ii) / c_ii.
1 / sqrt(c^_ii) = (1 / sigma_i)(1 - eta_i / 2 + ...), and the square root, the reciprocal, the product is_i is_j and the last product round once each.  So
    |r^_ij - r_ij| <= u (A_ij + |c_ij|) / (sigma_i sigma_j)  +  |r_ij| ((eps_i + eps_j) / 2 + 4u)        (first order; FIRST below).
FIRST counts 4u for the roundings behind c^; counted one by one they are 6 (two per reciprocal sigma, two products).  The tests allow TWICE FIRST: that holds
the 6u (8u >= 6u), the second-order terms (products of two of the relative errors above: eps_i is 2^-53 (A_ii + c_ii) / c_ii, about 2^-53 indiv = 2^-31 for a SNP
that is all 2s but for eight 1s among 4 194 304 individuals) and the reference's own roundings (a handful of 2^-64 relative to A + |c|, 2^-11 of the bound).
A float64 emulation of the three lines against this reference stayed below 0.985 FIRST for indiv from 3 to 50 000 and at near-constant rows at
indiv = 4 194 304; a single unit lost in one M_ij exceeds the bound by more than 10^8 there (1 / (sigma_i sigma_j) against u (A + c) / (sigma_i sigma_j)).
kind 1 stores fl(r^ r^): compared bit for bit with the square of the kind-0 value.

Scores.  score_i = sum over first[i] <= j <= last[i] of t(r_ij), t(r) = r^2 (plain) or r^2 - (1 - r^2) g, g = 1 / (indiv - 2) (adjusted; pairwise: g_ij =
1 / (N_ij - 2)).  Reference: math.fsum of the float64 values of t(r_ref) formed in long double.  Allowed error, with b_ij the element bound, m terms:
    m u sum_j |t_ij|                         any summation order of m float64 terms (test_ld_band_gpu.py)
  + sum_j (2 |r_ij| b_ij + b_ij^2)(1 + g)    t(r^) - t(r) = (1 + g)(r^^2 - r^2), exactly
  + 4u sum_j (|t_ij| + g)                    the term's own roundings: fl(r^ r^) moves t by u r^2 (1 + g), fl(1 - r2) by u g, fl(1 / (indiv - 2)) and the product
                                             (pairwise: the quotient) by 2u g, the subtraction by u |t|, the reference's conversion to float64 by u |t|; with
                                             r^2 <= |t| + g that is at most 3u |t| + 4u g.

Pairwise route: the restatement of mxa_ld_band_pairwise's definition (N, Sxy, Sx, Sy, Sxx, Syy as exact integers, r = num / sqrt(dx dy) in long double) with
its tolerance of 8 units of 2^-53 |r_ref| (test_ld_pairwise_gpu.py states why)."""
import math

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
PAIRWISE_UNITS = 8                       # |r - r_ref| <= 8 * 2^-53 * |r_ref| on the pairwise route


# ---------------------------------------------------------------------------------------------------------------------------------- decoding
def fields(X):
    """every 2-bit field of the packed rows, low bits first: rows x (4 * bytes per row) uint8, the padding fields of the last byte included"""
    P = np.ascontiguousarray(X, dtype=np.uint8)
    return np.stack([(P >> (2 * q)) & 3 for q in range(4)], axis=-1).reshape(P.shape[0], -1)


def codes(X, indiv):
    """the PLINK codes of the `indiv` individuals of every row"""
    return fields(X)[:, :indiv]


def staged(X, is_plink=True):
    """what the plain route multiplies: rows x (4 * bytes per row) uint8.  Raw: the fields.  PLINK: the byte table, a byte with a 01 field -> four 3s"""
    F = fields(X)
    if not is_plink:
        return F
    Z = np.where(F >= 2, F - 1, 0).astype(np.uint8)
    bad = (F.reshape(F.shape[0], -1, 4) == 1).any(axis=2)
    return np.where(np.repeat(bad, 4, axis=1), 3, Z).astype(np.uint8)


def gram_exact(Za, Zb=None, chunk=1 << 18, check_rows=3):
    """Za Zb^T (Zb = Za by default) of small non-negative integer matrices as float64 holding exact integers: float64 BLAS over K chunks (every partial sum
    is an integer below 9 K < 2^53), the first rows recomputed with numpy's int64 product"""
    Zb = Za if Zb is None else Zb
    K = Za.shape[1]
    assert Zb.shape[1] == K and 9.0 * K < 2.0 ** 53
    M = np.zeros((Za.shape[0], Zb.shape[0]))
    k = min(check_rows, Za.shape[0])
    Mi = np.zeros((k, Zb.shape[0]), np.int64)
    for k0 in range(0, K, chunk):
        M += Za[:, k0: k0 + chunk].astype(np.float64) @ Zb[:, k0: k0 + chunk].astype(np.float64).T
        Mi += Za[:k, k0: k0 + chunk].astype(np.int64) @ Zb[:, k0: k0 + chunk].T.astype(np.int64)
    assert np.array_equal(M[:k], Mi.astype(np.float64))
    return M


# -------------------------------------------------------------------------------------------------------------------------------- plain route
def ld_ref_pairs(Mij, Mii, Mjj, fi, fj, indiv, factor=2.0):
    """(r in long double, the allowed |r^ - r| = factor * FIRST of the module docstring in float64; inf where a sigma is 0) of the pairs whose exact
    crossproduct entries M_ij, M_ii, M_jj and float64 frequencies f_i, f_j are given as arrays of one shape"""
    fi, fj = np.asarray(fi, dtype=np.float64), np.asarray(fj, dtype=np.float64)
    n4 = LD(4.0 * indiv)
    cij = np.asarray(Mij).astype(LD) - n4 * (fi.astype(LD) * fj.astype(LD))
    cii = np.asarray(Mii).astype(LD) - n4 * (fi.astype(LD) * fi.astype(LD))
    cjj = np.asarray(Mjj).astype(LD) - n4 * (fj.astype(LD) * fj.astype(LD))
    with np.errstate(divide="ignore", invalid="ignore"):
        ss = np.sqrt(cii) * np.sqrt(cjj)
        r = cij / ss
        eps_i = U * (4.0 * indiv * fi * fi + cii.astype(np.float64)) / cii.astype(np.float64)
        eps_j = U * (4.0 * indiv * fj * fj + cjj.astype(np.float64)) / cjj.astype(np.float64)
        first = U * (4.0 * indiv * np.abs(fi * fj) + np.abs(cij).astype(np.float64)) / ss.astype(np.float64) + np.abs(r).astype(np.float64) * ((eps_i + eps_j) / 2 + 4 * U)
    return r, factor * np.where(np.isfinite(first) & (first > 0), first, np.inf)


def ld_ref(M, f, indiv):
    """(r, twice FIRST) of every (i, j) of the square exact crossproduct M"""
    d = np.diag(M)
    f = np.asarray(f, dtype=np.float64)
    return ld_ref_pairs(M, d[:, None], d[None, :], f[:, None], f[None, :], indiv)


def plain_case(X, indiv, f, is_plink=True):
    """dict(M, r (long double), b (the allowed |r^ - r|), sigma2 = diag c rounded to float64) of a packed matrix"""
    M = gram_exact(staged(X, is_plink))
    r, b = ld_ref(M, f, indiv)
    f = np.asarray(f, dtype=np.float64)
    return dict(M=M, r=r, b=b, sigma2=np.diag(M) - 4.0 * indiv * f * f)


def worst_ratio(got, r, b):
    """max |got - r| / b over the given entries (long double difference)"""
    if np.size(got) == 0:
        return 0.0
    err = np.abs(np.asarray(got).astype(LD) - r).astype(np.float64)
    with np.errstate(invalid="ignore"):
        q = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.max(q)) if np.all(np.isfinite(np.asarray(got))) else float("inf")


# ------------------------------------------------------------------------------------------------------------------------------------ windows
def pairs(last):
    """(ii, jj) of the stored entries in storage order: row i holds j = i .. last[i]"""
    n = len(last)
    cnt = np.asarray(last).astype(np.int64) - np.arange(n) + 1
    ii = np.repeat(np.arange(n), cnt)
    jj = ii + (np.arange(len(ii)) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    return ii, jj


def first_of(last):
    """first[i] = the smallest k with last[k] >= i (last is non-decreasing)"""
    return np.searchsorted(last, np.arange(len(last)), side="left")


def fixed_last(snps, w):
    return np.minimum(np.arange(snps) + w, snps - 1).astype(np.int32)


def rowptr_of(last):
    return np.concatenate([[0], np.cumsum(np.asarray(last).astype(np.int64) - np.arange(len(last)) + 1)]).astype(np.int64)


def window_bounds(pos, chrom, max_dist, max_snps=None):
    """the two-pointer sweep of mxa_ld_window_bounds restated: last[i] = the largest j >= i with chrom[j] == chrom[i], pos[j] - pos[i] <= max_dist (one
    rounded float64 subtraction) and j - i <= max_snps"""
    n = len(pos)
    last = np.empty(n, np.int32)
    j = 0
    for i in range(n):
        j = max(j, i)
        while j + 1 < n and chrom[j + 1] == chrom[i] and pos[j + 1] - pos[i] <= max_dist and (max_snps is None or j + 1 - i <= max_snps):
            j += 1
        last[i] = j
    return last, rowptr_of(last)


# ------------------------------------------------------------------------------------------------------------------------------------- scores
def score_terms(r, g):
    """t(r) in long double; g = 0 (plain), 1 / (indiv - 2), or the matrix 1 / (N_ij - 2)"""
    r2 = r * r
    return r2 - (1 - r2) * g


def score_row(r, b, g):
    """(reference score, allowed error) of one SNP from the long-double r, the element bounds b and g (scalar or per pair) of the pairs of its window"""
    g = np.broadcast_to(np.asarray(g, dtype=np.float64), np.shape(r))
    t = score_terms(r, g.astype(LD)).astype(np.float64)
    ra = np.abs(r).astype(np.float64)
    tol = len(t) * U * math.fsum(np.abs(t)) + math.fsum((2 * ra * b + b * b) * (1 + g)) + 4 * U * math.fsum(np.abs(t) + g)
    return math.fsum(t), tol


def scores_ref(r, b, g, last):
    """per SNP: (reference score, allowed error) over first[i] <= j <= last[i]; r long double (snps x snps), b the element bound, g as score_terms"""
    n = len(last)
    first = first_of(last)
    g = np.broadcast_to(np.asarray(g, dtype=np.float64), r.shape)
    ref, tol = np.empty(n), np.empty(n)
    for i in range(n):
        sl = slice(int(first[i]), int(last[i]) + 1)
        ref[i], tol[i] = score_row(r[i, sl], b[i, sl], g[i, sl])
    return ref, tol


# ----------------------------------------------------------------------------------------------------------------------------- pairwise route
def pairwise_restate(X, indiv, check_rows=16):
    """dict(N, Sxy: int64 snps x snps; r: long double, NaN where dx dy = 0) -- mxa_ld_band_pairwise's definition on the unpacked codes: m = present, z = allele
    count with missing as 0, a = code 11; N = M M^T, Sxy = Z Z^T, Sx = Z M^T, Sxx = Sx + 2 A M^T; num = N Sxy - Sx Sy, dx = N Sxx - Sx^2, dy = dx^T"""
    C = codes(X, indiv)
    M, Z, A = (C != 1).astype(np.uint8), np.where(C >= 2, C - 1, 0).astype(np.uint8), (C == 3).astype(np.uint8)

    def prod(P, Q):
        R = gram_exact(P, Q, check_rows=check_rows)                                                  # numpy's own int64 product on a block of rows
        Ri = R.astype(np.int64)
        assert np.array_equal(Ri, R)
        return Ri

    N, Sxy, Sx = prod(M, M), prod(Z, Z), prod(Z, M)
    Sxx = Sx + 2 * prod(A, M)
    Sy = Sx.T
    num = N * Sxy - Sx * Sy
    dx = N * Sxx - Sx * Sx
    assert dx.min() >= 0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = num.astype(LD) / np.sqrt(dx.astype(LD) * dx.T.astype(LD))
    return dict(N=N, Sxy=Sxy, r=r)


def pairwise_bound(r):
    return PAIRWISE_UNITS * U * np.abs(r).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------- seeded window geometries
SWEEP_REACHES = (0, 1, 30, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300, 10 ** 6)     # the last one: to the chromosome end


def sweep_window(snps, seed):
    """a seeded `last`: 1 to 6 chromosome ends at 32 k + o, o in {-2, -1, 0, 1}; runs of 1 to 96 consecutive SNPs, each run with one reach of SWEEP_REACHES;
    last = min(i + reach, chromosome end), running maximum, clipped to the chromosome end again"""
    rng = np.random.default_rng([snps, seed])
    ncut = int(rng.integers(1, 7))
    cuts = sorted({int(np.clip(32 * rng.integers(1, (snps + 31) // 32) + rng.integers(-2, 2), 0, snps - 2)) for _ in range(ncut)})
    ends = np.array(cuts + [snps - 1])                                               # the last SNP of each chromosome
    chrom_end = ends[np.searchsorted(ends, np.arange(snps), side="left")]
    reach = np.empty(snps, np.int64)
    i = 0
    while i < snps:
        ln = int(rng.integers(1, 97))
        reach[i: i + ln] = SWEEP_REACHES[int(rng.integers(len(SWEEP_REACHES)))]
        i += ln
    last = np.minimum(np.arange(snps) + reach, chrom_end)
    last = np.minimum(np.maximum.accumulate(last), chrom_end)                        # still non-decreasing: chrom_end is
    assert np.all(last >= np.arange(snps)) and np.all(np.diff(last) >= 0) and last[-1] == snps - 1
    return last.astype(np.int32)


SWEEP_EVENTS = ("sub-block skipped inside a listed tile", "sub-block kept by its last row only", "end on the first column of a sub-block",
                "end on the last column of a sub-block", "end on the first column of a tile", "end on the last column of a tile", "interior row of length 1",
                "tile rows of different length", "middle tile row with only its diagonal tile, reached from above")


def sweep_events(last):
    """which of SWEEP_EVENTS the window `last` holds, by the plan the header states: tile row I lists the 256 x 256 tiles (I, J), I <= J <= jmax[I] =
    last[min(256 I + 255, snps - 1)] // 256; inside a tile the 32 x 32 sub-block at (ib, jb) on or above the diagonal is skipped iff jb > last[its last row]"""
    n = len(last)
    nb = (n + 255) // 256
    jmax = [int(last[min(256 * I + 255, n - 1)]) // 256 for I in range(nb)]
    ev = set()
    if len({jmax[I] - I for I in range(nb - 1)}) > 1:
        ev.add("tile rows of different length")
    for I in range(nb):
        for J in range(I, jmax[I] + 1):
            for a in range(8):
                ib = 256 * I + 32 * a
                if ib >= n:
                    continue
                top = int(last[min(ib + 31, n - 1)])
                for b in range(8):
                    jb = 256 * J + 32 * b
                    if jb >= n or jb + 31 < ib:
                        continue
                    if jb > top:
                        ev.add("sub-block skipped inside a listed tile")
                    elif jb > int(last[ib]):
                        ev.add("sub-block kept by its last row only")
    if np.any(last % 32 == 0):
        ev.add("end on the first column of a sub-block")
    if np.any(last % 32 == 31):
        ev.add("end on the last column of a sub-block")
    if np.any(last % 256 == 0):
        ev.add("end on the first column of a tile")
    if np.any(last % 256 == 255):
        ev.add("end on the last column of a tile")
    if np.any((last - np.arange(n) == 0)[1:-1]):
        ev.add("interior row of length 1")
    if any(jmax[I] == I and jmax[I - 1] >= I for I in range(1, nb - 1)):
        ev.add("middle tile row with only its diagonal tile, reached from above")
    return ev
