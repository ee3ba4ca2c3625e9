"""References of the saddlepoint tests (mxa_assoc_score_spa).  numpy and math only; the library is imported by limits_operands alone.

spa_reference   the header's definition per (SNP, trait) in a chosen number type: np.longdouble run to |dt| <= 2^-45 |t| (a tighter stop does not converge
                in long double), or float64 with the entry's own stop rule.  Everything is computed from the operands: mu, U, V, z and a_j as plain sums in
                that type, g, the four sums, Newton with its bracket on both sides, the Lugannani-Rice / Barndorff-Nielsen tail
exact_two_sided the exact two-sided p-value of U = sum x_i (y_i - p_i) for integer genotypes without covariates (kh = 0): the distribution of sum x_i y_i
                with independent y_i ~ Bernoulli(p_i), by convolution over the carriers
rare_case       binary_case of tests/_assoc_score_ref.py with 3-5 % cases and every fourth SNP at MAF 0.01
null_operands   rare_case with the null models fitted by the library module handed in: the operands of the entry

For tests/test_assoc_spa_limits_{cpu,gpu}.py:
checked_references  both references of one case after the conditions on the inputs (equal flags, no |z| at the cutoff, no support margin at 2^-30 A, a cap on
                the evaluations), with eps = the largest |log p_64 - log p_LD|
loud_and_quiet  the rows of a pool that are marked (two traits, one trait) and the rows that are not
boundary_layouts    1030 positions filled with pool rows so that the marks fall on the 256-SNP rounds of the device's compaction
tail_operands   null_operands with six rows overwritten by SNPs that all or part of the cases carry: p-values down to the underflow of erfc
tail_errors     the relative rule for log p in that tail
"""
import functools
import math

import numpy as np

from _assoc_ref import LD, genotypes, pack  # noqa: F401
from _assoc_score_ref import score_sums

TOL_LD = 2.0 ** -45
OUTSIDE, FAILED, SOLVED = 0, 1, 2
_TWO_OVER_SQRT_PI = 2.0 / math.sqrt(math.pi)


def erfc_of(x, T):
    """erfc(x) in the type T: math.erfc at the nearest double, and for long double the first-order term of what the rounding of x dropped"""
    xd = float(x)
    if T is not LD:
        return T(math.erfc(xd))
    rest = float(LD(x) - LD(xd))
    return LD(math.erfc(xd)) - LD(_TWO_OVER_SQRT_PI * math.exp(-min(xd * xd, 740.0))) * LD(rest)


def normal_p(z, T=np.float64):
    return erfc_of(abs(T(z)) / np.sqrt(T(2)), T)


def cgf(t, g, p, c0):
    """K(t), K'(t), K''(t) of the centred statistic in the overflow-free form of the header"""
    x = t * g
    e = np.exp(-np.abs(x))
    pos = x >= 0
    al, be = np.where(pos, p, 1 - p), np.where(pos, 1 - p, p)
    d = al + be * e
    K = (np.maximum(x, 0) + np.log(d)).sum() - t * c0
    K1 = (g * np.where(pos, p / d, p * e / d)).sum() - c0
    K2 = (g * g * al * be * e / (d * d)).sum()
    return K, K1, K2


def solve_side(g, p, c0, A, G_side, absU, sigma, tol, max_iter, T):
    """(status, tail, evaluations of the Newton loop, support margin sigma (b - q)); the evaluation at the accepted t^ itself is not counted"""
    q = T(sigma) * absU
    b = G_side - c0
    margin = T(sigma) * (b - q)
    if margin <= T(2.0 ** -30) * A:
        return OUTSIDE, None, 0, margin
    t, lo, hi, that, evals = T(0), T(-np.inf), T(np.inf), None, 0
    with np.errstate(all="ignore"):
        while evals < max_iter:
            _, K1, K2 = cgf(t, g, p, c0)
            evals += 1
            f = K1 - q
            if f < 0:
                lo = t
            else:
                hi = t
            tn = t - f / K2
            if not np.isfinite(tn):
                return FAILED, None, evals, margin
            if abs(tn - t) <= T(tol) * abs(tn):
                that = tn
                break
            if not (lo < tn < hi):
                tn = (lo + hi) / 2
                if not np.isfinite(tn):
                    return FAILED, None, evals, margin
            t = tn
        if that is None:
            return FAILED, None, evals, margin
        K, _, K2 = cgf(that, g, p, c0)
        w = np.sign(that) * np.sqrt(2 * (that * q - K))
        v = that * np.sqrt(K2)
        zeta = w + np.log(v / w) / w
        if not np.isfinite(zeta):
            return FAILED, None, evals, margin
    return SOLVED, T(0.5) * erfc_of(T(sigma) * zeta / np.sqrt(T(2)), T), evals, margin


def spa_item(x, p, tau, a, U, z, tol, max_iter, T):
    """(flag, pval, evaluations, [margins / A of both sides]) of one item that is to be corrected.  x: the allele counts with mu at the missing calls, tau:
    (kh, indiv) = h / w, a: (kh,)"""
    g = x.astype(T).copy()
    for j in range(len(a)):
        g = g - a[j] * tau[j]                       # (the fma of the definition: one rounding less, below what the tolerance resolves)
    c0, A = (g * p).sum(), np.abs(g).sum()
    Gp, Gm = np.maximum(g, 0).sum(), np.minimum(g, 0).sum()
    obs = 1 if U >= 0 else -1
    res = {s: solve_side(g, p, c0, A, Gp if s > 0 else Gm, abs(U), s, tol, max_iter, T) for s in (1, -1)}
    evals = max(r[2] for r in res.values())
    margins = [float(r[3] / A) if A > 0 else 0.0 for r in res.values()]
    if res[obs][0] != SOLVED or res[-obs][0] == FAILED:
        return 2, normal_p(z, T), evals, margins
    return 1, res[obs][1] + (res[-obs][1] if res[-obs][0] == SOLVED else T(0)), evals, margins


def spa_reference(codes, P, R, Wt, H, z_cutoff=2.0, tol=2.0 ** -30, max_iter=50, T=np.float64):
    """pval (snps, n) in T, flag (snps, n) int32, z (snps, n) in T, evals (snps, n) and the list of support margins / A of the corrected items"""
    codes = np.asarray(codes)
    snps, indiv = codes.shape
    n = R.shape[1]
    kh = H.shape[1] // n if n else 0
    with np.errstate(all="ignore"):
        N, Sz, D, M, E = score_sums(codes, R, Wt, H, T)
        mu = Sz.astype(T) / N.astype(T)
        a_all = mu[:, None] * M + D
        pval, flag, evals = np.full((snps, n), np.nan, T), np.zeros((snps, n), np.int32), np.zeros((snps, n), np.int32)
        zs = np.full((snps, n), np.nan, T)
        margins = []
        Pt, Wtt, Ht = np.asarray(P).astype(T), np.asarray(Wt).astype(T), np.asarray(H).astype(T)
        for c in range(n):
            tau = (Ht[:, c * kh:(c + 1) * kh] / Wtt[:, c:c + 1]).T if kh else np.zeros((0, indiv), T)
            for s in range(snps):
                a = a_all[s, 2 * n + c * kh: 2 * n + (c + 1) * kh]
                U = a_all[s, c]
                V = D[s, n + c] + 2 * E[s, c] + mu[s] * mu[s] * M[s, n + c] - (a * a).sum()
                z = U / np.sqrt(V)
                zs[s, c] = z
                if not np.isfinite(z):
                    flag[s, c] = 3
                elif abs(z) < z_cutoff:
                    pval[s, c] = normal_p(z, T)
                else:
                    x = np.where(codes[s] < 0, mu[s], np.maximum(codes[s], 0).astype(T))
                    flag[s, c], pval[s, c], evals[s, c], m = spa_item(x, Pt[:, c], tau, a, U, z, tol, max_iter, T)
                    margins.extend(m)
    return pval, flag, zs, evals, margins


def exact_two_sided(x, p, U):
    """P(|T - E T| >= |U|) for T = sum x_i y_i, y_i ~ Bernoulli(p_i) independent, x_i in {0, 1, 2}: the distribution by convolution over the carriers in
    np.longdouble, the two tails summed from their small ends.  A lattice point counts as reached within 1e-9 (the mean is a sum of doubles)."""
    x = np.asarray(x, np.int64)
    p = np.asarray(p).astype(LD)
    dist = np.zeros(int(x.sum()) + 1, LD)
    dist[0] = 1
    top = 0
    for xi, pi in zip(x[x > 0], p[x > 0]):
        new = dist[:top + xi + 1] * (1 - pi)
        new[xi:] += dist[:top + 1] * pi
        top += xi
        dist[:top + 1] = new
    dev = np.arange(len(dist)).astype(LD) - (x.astype(LD) * p).sum()
    au = abs(LD(U)) - LD(1e-9)
    upper, lower = dist[dev >= au], dist[dev <= -au]
    return float(upper[::-1].sum() + lower.sum())


def rare_case(indiv, snps, n, q, seed):
    """(codes, Y, W): binary_case of tests/_assoc_score_ref.py at a case fraction of 0.03-0.05 (by the seed), with every fourth SNP redrawn at MAF 0.01 and
    5 % missing calls like the others.  Every trait keeps at least three cases and three controls."""
    from _assoc_score_ref import binary_case
    rng = np.random.default_rng([seed, indiv, snps, n, q, 11])
    fraction = float(rng.uniform(0.03, 0.05))
    codes, Y, W = binary_case(indiv, snps, n, q, seed, fraction=fraction)
    codes = codes.copy()
    for s in range(0, snps, 4):
        row = rng.binomial(2, 0.01, indiv).astype(np.int8)
        if not np.any(row > 0):
            row[int(rng.integers(0, indiv))] = 1
        row[rng.random(indiv) < 0.05] = -1
        if not np.any(row > 0):
            row[int(rng.integers(0, indiv))] = 1
        codes[s] = row
    Y = np.array(Y, order="F")
    for c in range(n):
        Y[:3, c] = 1.0
        Y[3:6, c] = 0.0
    return codes, Y, np.asfortranarray(W)


def null_operands(mx, indiv, snps, n, kh, seed):
    """(codes, packed rows, Y, W, P, R, Wt, H) of rare_case(indiv, snps, n, q = max(kh - 1, 0), seed): the null of every trait fitted by mx.assoc_logistic_null
    (mx: the library's Python package), P = Y - R; kh = 0: the same nulls without projection columns (H has no column)"""
    q = max(kh - 1, 0)
    codes, Y, W = rare_case(indiv, snps, n, q, seed)
    fits = [mx.assoc_logistic_null(Y[:, c], W if q else None) for c in range(n)]
    R, Wt, H = (np.asfortranarray(np.concatenate([np.reshape(getattr(f, k), (indiv, -1)) for f in fits], axis=1)) for k in ("r", "w", "H"))
    if kh == 0:
        H = np.zeros((indiv, 0), order="F")
    return codes, pack(codes), Y, W, np.asfortranarray(Y - R), R, Wt, H


# ---- tests/test_assoc_spa_limits_{cpu,gpu}.py: the cases, each built once per process and read-only
LIMITS_SEED = 3
#             indiv snps n kh z_cutoff
LIST_CASES = [(67, 700, 3, 1, 0.5), (259, 300, 8, 2, 1.0), (259, 33, 3, 10, 1.0)]
MAX_ITER_CASE = (259, 300, 8, 2, 1.0)
LOOSE_TOL_CASE, LOOSE_TOL = (259, 130, 3, 3, 2.0), 2.0 ** -12
POOL_CASE = (67, 130, 2, 1, 1.5)
ROUNDS_TOTAL = 1030                     # four full rounds of 256 SNPs and a last one of 6
TAIL_INDIV = (1027, 4099, 8195)
#            fraction of the cases, their allele count, controls at the count 1
TAIL_ROWS = [(1.0, 2, 3), (1.0, 1, 3), (0.5, 2, 5), (0.25, 2, 10), (1.0, 2, 40), (0.75, 1, 1)]
TAIL_FLOOR = 1e-290


def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def limits_operands(indiv, snps, n, kh):
    """null_operands of the library in this tree at LIMITS_SEED (the one place of this file that imports it)"""
    import miraculix_amd as mx
    mx.load_shared_library()
    return frozen(*null_operands(mx, indiv, snps, n, kh, LIMITS_SEED))


def log_eps(p64, pld, floor=1e-200):
    ok = np.isfinite(pld.astype(np.float64)) & (pld > floor)
    return float(np.abs(np.log(p64[ok].astype(LD)) - np.log(pld[ok])).max()) if ok.any() else 0.0


def checked_references(codes, P, R, Wt, H, z_cutoff, tol=2.0 ** -30, max_iter=50, tol_ld=TOL_LD, cap=20):
    """dict(p64, pld, flags, z, e64, eld, eps) of both references after the conditions on the inputs: the flags of the two are equal, no |z| lies within
    2^-40 z_cutoff of the cutoff, no support margin in [2^-31, 2^-29] A, and neither reference needs more than cap evaluations on a side"""
    p64, f64, z64, e64, _ = spa_reference(codes, P, R, Wt, H, z_cutoff, tol, max_iter, np.float64)
    pld, fld, _, eld, margins = spa_reference(codes, P, R, Wt, H, z_cutoff, tol_ld, 200, LD)
    assert np.array_equal(f64, fld), np.argwhere(f64 != fld)[:5]
    fin = np.isfinite(z64)
    assert not np.any(np.abs(np.abs(z64[fin]) - z_cutoff) <= 2.0 ** -40 * z_cutoff)
    m = np.array(margins)
    assert not np.any((m >= 2.0 ** -31) & (m <= 2.0 ** -29))
    assert max(e64.max(), eld.max()) <= cap, (e64.max(), eld.max())
    out = dict(p64=p64, pld=pld, flags=f64, z=z64, e64=e64, eld=eld)
    frozen(*out.values())
    out["eps"] = log_eps(p64, pld)
    return out


@functools.lru_cache(maxsize=None)
def limits_reference(indiv, snps, n, kh, z_cutoff, tol=2.0 ** -30, tol_ld=TOL_LD):
    codes, _, _, _, P, R, Wt, H = limits_operands(indiv, snps, n, kh)
    return checked_references(codes, P, R, Wt, H, z_cutoff, tol, 50, tol_ld)


def batch_cuts(off, max_items, max_rows):
    """the batches [k0, k1) of the entry's rule over the item offsets off (len = marked SNPs + 1), and per batch what ended it: 'rows', 'items' or 'end'"""
    nk = len(off) - 1
    max_items, max_rows = min(max_items, int(off[nk])), min(max_rows, nk)
    out, k0 = [], 0
    while k0 < nk:
        k1 = k0 + 1
        while k1 < nk and k1 - k0 < max_rows and off[k1 + 1] - off[k0] <= max_items:
            k1 += 1
        out.append((k0, k1, "end" if k1 == nk else "rows" if k1 - k0 >= max_rows else "items"))
        k0 = k1
    return out


def item_offsets(flags):
    """off of the device's list: the exclusive prefix sums of the marks per marked SNP, the total appended"""
    cnt = (np.asarray(flags) == 1).sum(axis=1)
    return np.concatenate([[0], np.cumsum(cnt[cnt > 0])])


def loud_and_quiet(flags):
    """(rows with both traits marked, rows with one trait marked and the other at 0, rows with every trait at 0) of a pool's flags (rows, 2)"""
    marked, other = (flags == 1), (flags >= 2)
    loud = marked.any(axis=1) & ~other.any(axis=1)
    return np.flatnonzero(loud & marked.all(axis=1)), np.flatnonzero(loud & ~marked.all(axis=1)), np.flatnonzero((flags == 0).all(axis=1))


def boundary_layouts(two, one, quiet, missing, total=ROUNDS_TOTAL):
    """name -> the pool row of each of `total` positions.  The loud positions take two-item and one-item rows in turn (each kind cycled), the others the quiet
    rows cycled; `missing` is the pool's entirely missing row"""
    def fill(loud_at, missing_at=()):
        is_loud = np.zeros(total, bool)
        is_loud[list(loud_at)] = True
        lay, j, q = np.empty(total, np.int64), 0, 0
        for pos in range(total):
            if is_loud[pos]:
                src = two if j % 2 == 0 else one
                lay[pos] = src[(j // 2) % len(src)]
                j += 1
            else:
                lay[pos] = quiet[q % len(quiet)]
                q += 1
        lay[list(missing_at)] = missing
        return lay
    return {"edges": fill((0, 255, 256, 511, 512, total - 1), (254, 768)),
            "empty_and_full": fill(list(range(256, 512)) + [total - 1]),
            "all_loud": fill(range(total)),
            "alternating": fill(range(1, total, 2))}


@functools.lru_cache(maxsize=None)
def pool():
    """dict: the pool's codes with an entirely missing row appended (index `missing`), the operands, both references of the pool (checked_references), the
    three kinds of rows and the layouts"""
    indiv, snps, n, kh, z_cutoff = POOL_CASE
    codes, _, Y, W, P, R, Wt, H = limits_operands(indiv, snps, n, kh)
    codes = np.concatenate([codes, np.full((1, indiv), -1, codes.dtype)])
    ref = checked_references(codes, P, R, Wt, H, z_cutoff)
    two, one, quiet = loud_and_quiet(ref["flags"][:snps])
    frozen(codes)
    return dict(codes=codes, operands=(P, R, Wt, H), z_cutoff=z_cutoff, ref=ref, two=two, one=one, quiet=quiet, missing=snps,
                layouts=boundary_layouts(two, one, quiet, snps))


@functools.lru_cache(maxsize=None)
def tail_operands(indiv):
    """limits_operands(indiv, 24, 1, 1) with the rows of TAIL_ROWS written over the first six: no missing call, the first round(fraction cases) cases at the
    allele count, the drawn controls at 1, everyone else at 0"""
    codes, _, Y, W, P, R, Wt, H = limits_operands(indiv, 24, 1, 1)
    codes = codes.copy()
    cases, controls = np.flatnonzero(Y[:, 0] > 0), np.flatnonzero(Y[:, 0] == 0)
    rng = np.random.default_rng([LIMITS_SEED, indiv, 5])
    for row, (fraction, count, at_one) in enumerate(TAIL_ROWS):
        codes[row] = 0
        codes[row, cases[:int(round(fraction * len(cases)))]] = count
        codes[row, rng.choice(controls, at_one, replace=False)] = 1
    return frozen(codes, pack(codes)) + (Y, W, P, R, Wt, H)


@functools.lru_cache(maxsize=None)
def tail_reference(indiv):
    codes, _, _, _, P, R, Wt, H = tail_operands(indiv)
    ref = checked_references(codes, P, R, Wt, H, 1.0)
    ref["eps_rel"] = tail_errors(ref["p64"], ref["p64"], ref["pld"])
    return ref


def tail_errors(got, p64, pld):
    """the largest |log got - log p_LD| / max(1, |log p_LD|) over the entries with p_LD > TAIL_FLOOR, after the rules for the rest: NaNs where the
    reference's are; where the float64 reference is exactly 0, finite, not negative and below 1e-300; reference values in (0, TAIL_FLOOR]: within [0, 1e-280]"""
    got, pd = np.asarray(got, np.float64), pld.astype(np.float64)
    nan = np.isnan(pd)
    assert np.array_equal(np.isnan(got), nan)
    ok = ~nan & (pld > TAIL_FLOOR)
    assert np.all(got[ok] > 0)
    zero = ~nan & (p64 == 0)
    assert not np.any(zero & ok)
    assert np.all(np.isfinite(got[zero]) & (got[zero] >= 0) & (got[zero] < 1e-300)), got[zero]
    low = ~nan & ~ok & ~zero
    assert np.all((got[low] >= 0) & (got[low] <= 1e-280)), got[low]
    logs = np.log(pld[ok])
    return float((np.abs(np.log(got[ok].astype(LD)) - logs) / np.maximum(1, np.abs(logs))).max())
