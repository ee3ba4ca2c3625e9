"""References of the mxa_ld_window_apply tests: plain numpy, nothing of the library is imported.

Y = T_w(R) X with Y[i, c] = sum over first[i] <= j <= last[i] of T[i, j] X[j, c].  The tests take T from the BITS the rows entries store at kind 0, so the new
kernels are tested apart from the r map:
    terms(R, indiv, term)      plain route: 0 -> r, 1 -> fl(r r), 2 -> r2 - (1 - r2) (1 / (indiv - 2)), in the kernel's operation order
    terms_pw(R, N, term)       pairwise route: 2 -> r2 - ((1 - r2) / (N_ij - 2)) with the exact integer N_ij of present_counts()
    dense(values, last)        the ragged rows as a symmetric snps x snps matrix, NaN outside the window
    apply_ref(T, last, X)      (ref, mag, m): ref[i, c] = math.fsum of the float64 products T[i, j] X[j, c], mag[i, c] = sum |T[i, j] X[j, c]|, m[i] = the
                               number of terms.  mag is numpy's sum scaled by 1 - 2^-40, i.e. a little BELOW the true sum (numpy's pairwise sum of m
                               non-negative terms is off by far less than 2^-40 relative), so a bound built on it asks no less than one built on the true sum.
The windows: the chromosome and cluster families of test_ld_window_var_gpu.py restated on _ld_ref.window_bounds (the two-pointer sweep in numpy)."""
import math

import numpy as np

import _ld_ref as ref

U = 2.0 ** -53
NC = 16                                    # columns per workgroup of the tile kernel (miraculix_amd.crossproduct.LD_APPLY_NC)
TERMS = ("r", "r2", "r2_adj")
CHROM_LENGTHS = (1, 255, 256, 257, 511, 1, 700)


def chromosome_window(snps):
    """chromosomes of lengths 1, 255, 256, 257, 511, 1, 700 and the rest (cut where snps ends), positions 1000 k inside each, max_dist 300 000"""
    lengths, left = [], snps
    for ln in CHROM_LENGTHS:
        if left > 0:
            lengths.append(min(ln, left))
            left -= lengths[-1]
    if left > 0:
        lengths.append(left)
    chrom = np.repeat(np.arange(len(lengths)), lengths).astype(np.int32)
    pos = np.concatenate([1000.0 * np.arange(ln) for ln in lengths])
    last, _ = ref.window_bounds(pos, chrom, 300_000.0)
    ends = np.cumsum(lengths) - 1
    assert np.array_equal(last[ends], ends)
    return last


def cluster_window(snps, seed=17):
    """seeded gaps, 30 % of them 0 (ties) and 15 % above max_dist, and a run of SNPs at one position from index 200 on: reaches from 0 to beyond two tiles"""
    rng = np.random.default_rng(seed)
    max_dist = 1.0
    gaps = rng.exponential(max_dist / 25.0, size=snps)
    gaps[rng.random(snps) < 0.3] = 0.0
    gaps[rng.random(snps) < 0.15] = max_dist * (1.0 + rng.random())
    run = min(600, snps - 201)
    assert run > 1, "the cluster family needs more than 202 SNPs"
    gaps[201: 200 + run] = 0.0
    gaps[200] = gaps[200 + run] = 2.0 * max_dist
    pos = np.cumsum(gaps)
    last, _ = ref.window_bounds(pos, np.zeros(snps, np.int32), max_dist)
    reach = last - np.arange(snps)
    assert reach.min() == 0 and reach[200] == run - 1
    return last


def terms(R, indiv, term):
    if term == 0:
        return R
    r2 = R * R
    if term == 1:
        return r2
    return r2 - (1.0 - r2) * (1.0 / (float(indiv) - 2.0))


def terms_pw(R, N, term):
    if term == 0:
        return R
    r2 = R * R
    if term == 1:
        return r2
    with np.errstate(divide="ignore", invalid="ignore"):
        return r2 - (1.0 - r2) / (N - 2.0)


def present_counts(X, indiv):
    """N_ij = individuals genotyped at both SNPs, exact: the fp64 product of 0 / 1 matrices sums integers below 2^53"""
    M = (ref.codes(X, indiv) != 1).astype(np.float64)
    N = M @ M.T
    k = min(8, len(M))
    assert np.array_equal(N[:k], (M[:k].astype(np.int64) @ M.T.astype(np.int64)).astype(np.float64))
    return N


def dense(values, last):
    """the ragged rows (row i: j = i .. last[i]) as a symmetric matrix, NaN outside the window"""
    n = len(last)
    ii, jj = ref.pairs(last)
    assert len(values) == len(ii)
    R = np.full((n, n), np.nan)
    R[ii, jj] = values
    R[jj, ii] = values
    return R


def apply_ref(T, last, X):
    """(ref, mag, m) of the module docstring; X: snps x n"""
    n = len(last)
    first = ref.first_of(last)
    X = np.asarray(X, dtype=np.float64).reshape(n, -1)
    out, mag = np.empty(X.shape), np.empty(X.shape)
    for i in range(n):
        lo, hi = int(first[i]), int(last[i]) + 1
        prod = T[i, lo:hi, None] * X[lo:hi]                                       # float64 products, one rounding each
        out[i] = [math.fsum(col) for col in prod.T.tolist()]
        mag[i] = np.abs(prod).sum(axis=0)
    return out, mag * (1.0 - 2.0 ** -40), (np.asarray(last) - first + 1).astype(np.float64)


def dense_apply_longdouble(T, last, X):
    """W @ X in long double with W = T inside the window and 0 outside: the independent restatement apply_ref is checked against"""
    n = len(last)
    first = ref.first_of(last)
    j = np.arange(n)
    inside = (j[None, :] >= first[:, None]) & (j[None, :] <= np.asarray(last)[:, None])
    W = np.where(inside, T, 0.0).astype(np.longdouble)
    return W @ np.asarray(X, dtype=np.float64).reshape(n, -1).astype(np.longdouble)
