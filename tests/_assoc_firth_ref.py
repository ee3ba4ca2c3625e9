"""References of the effect-size tests (mxa_assoc_score_firth).  numpy and math only; cgf, erfc_of, normal_p, rare_case and null_operands are those of
tests/_assoc_spa_ref.py, unchanged.

cgf4             K', K'', K''', K'''' of the header at one beta, in the type of its operands
fit              the header's Newton loop on one adjusted genotype g: (status, beta^, K(beta^), K''(beta^), K''(0), evaluations, support margin / A)
firth_item       flag, beta, se, chisq, pval of one item that is to be fitted
firth_reference  the header's definition per (SNP, trait) in a chosen number type: np.longdouble run to |d beta| <= 2^-45 |beta|, or float64 with the entry's
                 own stop rule.  Everything is computed from the operands, as spa_reference does
both_references  the two of one case after the conditions on the inputs, with eps = the largest difference of the two over the fitted cells: relative in
                 beta and se, in chisq / max(1, chisq), and in log pval
penalised_loglik the penalised log likelihood of logit pi = logit p + beta g evaluated from y: sum [y log pi + (1 - y) log(1 - pi)] + (penalty / 2) log sum g^2
                 pi (1 - pi), with the sum of the absolute values of its terms

For tests/test_assoc_firth_limits_{cpu,gpu}.py (the second half of the file): fit, firth_item and firth_reference take an optional `trace` that records the
decisions of every evaluation and changes no result; limit_errors (errors with beta^ = 0 and without log pval in the tail), limits_references (both_references
plus the two traces), and the builders of the cases on limits_operands, tail_operands, TAIL_ROWS and LIST_CASES of tests/_assoc_spa_ref.py: bisect_operands,
alt_operands, negative_operands, saturated_operands, zero_operands, limits_case / limits_reference (each case once per process), max_iter_flags.
"""
import functools

import numpy as np

from _assoc_score_ref import score_sums
from _assoc_spa_ref import FAILED, LD, OUTSIDE, SOLVED, TOL_LD, erfc_of, cgf, normal_p  # noqa: F401
from _assoc_spa_ref import LIMITS_SEED, LIST_CASES, TAIL_ROWS, batch_cuts, frozen, item_offsets, limits_operands, pack, tail_errors, tail_operands  # noqa: F401

FLOOR = 1e-200                              # p-values below it are not compared in log pval


def cgf4(b, g, p, c0):
    x = b * g
    e = np.exp(-np.abs(x))
    pos = x >= 0
    al, be = np.where(pos, p, 1 - p), np.where(pos, 1 - p, p)
    d = al + be * e
    pi = np.where(pos, p / d, p * e / d)
    om = al * be * e / (d * d)
    g2 = g * g
    return (g * pi).sum() - c0, (g2 * om).sum(), (g2 * g * om * (1 - 2 * pi)).sum(), (g2 * g2 * om * (1 - 6 * om)).sum()


def fit(g, p, U, penalty, tol, max_iter, T, trace=None):
    """trace: a list that receives one dict for this fit (see the head of the limits part below); the results do not depend on it"""
    c0, A = (g * p).sum(), np.abs(g).sum()
    tr = None
    if trace is not None:
        tr = dict(beta=[], replaced=[], ratio=[], bisected=[], edge=[], reach=[], status=OUTSIDE, evals=0, chisq=None)
        trace.append(tr)
        carried = np.abs(g[g != 0]).max() if np.any(g != 0) else T(0)
    sigma = 1 if U >= 0 else -1             # (the margin is reported for both penalties; only penalty == 0 acts on it)
    b = (np.maximum(g, 0).sum() if sigma > 0 else np.minimum(g, 0).sum()) - c0
    margin = T(sigma) * (b - U)
    rel = float(margin / A) if A > 0 else 0.0
    if penalty == 0 and margin <= T(2.0 ** -30) * A:
        return OUTSIDE, None, None, None, None, 0, rel

    def ended(status):
        if tr is not None:
            tr.update(status=status, evals=evals)
        return status
    beta, lo, hi, hat, evals, k20 = T(0), T(-np.inf), T(np.inf), None, 0, None
    with np.errstate(all="ignore"):
        while evals < max_iter:
            K1, K2, K3, K4 = cgf4(beta, g, p, c0)
            evals += 1
            if evals == 1:
                k20 = K2
            f, fp = K1 - U, K2
            alt = None
            if penalty:
                r3 = K3 / K2
                f = f - T(0.5) * r3
                alt = K2 - T(0.5) * (K4 / K2 - r3 * r3)
                if alt > 0:
                    fp = alt
            if f < 0:
                lo = beta
            else:
                hi = beta
            bn = beta - f / fp
            if tr is not None:
                tr["beta"].append(float(beta))
                tr["reach"].append(float(abs(beta) * carried))
                tr["replaced"].append(bool(penalty) and not alt > 0)
                tr["ratio"].append(float(alt / K2) if penalty else np.nan)
                tr["bisected"].append(False)
                tr["edge"].append(np.nan)
            if not np.isfinite(bn):
                return ended(FAILED), None, None, None, None, evals, rel
            if abs(bn - beta) <= T(tol) * abs(bn):
                hat = bn
                break
            if tr is not None:                  # (only here does the loop decide between the Newton beta' and the middle of the bracket)
                tr["edge"][-1] = float(abs((hi if f < 0 else lo) - bn) / abs(bn))
                tr["bisected"][-1] = not lo < bn < hi
            if not (lo < bn < hi):
                bn = (lo + hi) / 2
                if not np.isfinite(bn):
                    return ended(FAILED), None, None, None, None, evals, rel
            beta = bn
        if hat is None:
            return ended(FAILED), None, None, None, None, evals, rel
        K, _, K2 = cgf(hat, g, p, c0)
    ended(SOLVED)
    return SOLVED, hat, K, K2, k20, evals, rel


def one_step(U, V, z, T):
    with np.errstate(all="ignore"):
        return U / V, 1 / np.sqrt(V), z * z, normal_p(z, T)


def results_of_fit(res, U, V, z, penalty, T, tr=None):
    """(flag, beta, se, chisq, pval) from fit's result; tr: the fit's dict of the trace, which receives the chisq before max(0, .)"""
    status, hat, K, K2, k20 = res[:5]
    if status == SOLVED:
        with np.errstate(all="ignore"):
            se = 1 / np.sqrt(K2)
            x2 = 2 * (hat * U - K)
            if penalty:
                x2 = x2 + np.log(K2 / k20)
        if tr is not None:
            tr["chisq"] = x2
        if np.isfinite(se) and np.isfinite(x2):
            x2 = max(x2, T(0))
            return 1, hat, se, x2, erfc_of(np.sqrt(x2 / 2), T)
    return (2,) + one_step(U, V, z, T)


def firth_item(x, p, tau, a, U, V, z, penalty, tol, max_iter, T, trace=None):
    """(flag, beta, se, chisq, pval, evaluations, support margin / A) of one item that is to be fitted.  x: the allele counts with mu at the missing calls,
    tau: (kh, indiv) = h / w, a: (kh,)"""
    g = x.astype(T).copy()
    for j in range(len(a)):
        g = g - a[j] * tau[j]
    res = fit(g, p, U, penalty, tol, max_iter, T, trace)
    return results_of_fit(res, U, V, z, penalty, T, trace[-1] if trace is not None else None) + (res[5], res[6])


def firth_reference(codes, P, R, Wt, H, z_cutoff=2.0, penalty=1, tol=2.0 ** -30, max_iter=50, T=np.float64, trace=None):
    """dict of beta, se, chisq, pval, z (snps, n) in T, flag and evals (snps, n) int32, and margins: the support margins / A of the fitted items.  trace: a
    list that receives fit's dict of every item in the order of the fits, with cell = (s, c), the item's U and its margin / A"""
    codes = np.asarray(codes)
    snps, indiv = codes.shape
    n = R.shape[1]
    kh = H.shape[1] // n if n else 0
    out = {k: np.full((snps, n), np.nan, T) for k in ("beta", "se", "chisq", "pval", "z")}
    flag, evals, margins = np.zeros((snps, n), np.int32), np.zeros((snps, n), np.int32), []
    with np.errstate(all="ignore"):
        N, Sz, D, M, E = score_sums(codes, R, Wt, H, T)
        mu = Sz.astype(T) / N.astype(T)
        a_all = mu[:, None] * M + D
        Pt, Wtt, Ht = np.asarray(P).astype(T), np.asarray(Wt).astype(T), np.asarray(H).astype(T)
        for c in range(n):
            tau = (Ht[:, c * kh:(c + 1) * kh] / Wtt[:, c:c + 1]).T if kh else np.zeros((0, indiv), T)
            for s in range(snps):
                a = a_all[s, 2 * n + c * kh: 2 * n + (c + 1) * kh]
                U = a_all[s, c]
                V = D[s, n + c] + 2 * E[s, c] + mu[s] * mu[s] * M[s, n + c] - (a * a).sum()
                z = U / np.sqrt(V)
                out["z"][s, c] = z
                if not np.isfinite(z):
                    flag[s, c] = 3
                    continue
                if abs(z) < z_cutoff:
                    got = (0,) + one_step(U, V, z, T)
                else:
                    x = np.where(codes[s] < 0, mu[s], np.maximum(codes[s], 0).astype(T))
                    got = firth_item(x, Pt[:, c], tau, a, U, V, z, penalty, tol, max_iter, T, trace)
                    if trace is not None:
                        trace[-1].update(cell=(s, c), U=float(U), margin=got[6])
                    evals[s, c] = got[5]
                    margins.append(got[6])
                flag[s, c] = got[0]
                for k, v in zip(("beta", "se", "chisq", "pval"), got[1:5]):
                    out[k][s, c] = v
    out.update(flag=flag, evals=evals, margins=margins)
    return out


def errors(got, ref, cells):
    """the four measures of got against ref (dicts of arrays) over the cells of the boolean mask: relative in beta and se, in chisq / max(1, chisq), in log pval
    (where the reference p-value exceeds FLOOR)"""
    def over(v):
        return float(v.max()) if v.size else 0.0
    g = {k: np.asarray(got[k])[cells].astype(LD) for k in ("beta", "se", "chisq", "pval")}
    r = {k: np.asarray(ref[k])[cells].astype(LD) for k in ("beta", "se", "chisq", "pval")}
    ok = r["pval"] > FLOOR
    assert np.all(g["pval"][ok] > 0)
    return {"beta": over(np.abs(g["beta"] - r["beta"]) / np.abs(r["beta"])), "se": over(np.abs(g["se"] - r["se"]) / r["se"]),
            "chisq": over(np.abs(g["chisq"] - r["chisq"]) / np.maximum(1, r["chisq"])), "pval": over(np.abs(np.log(g["pval"][ok]) - np.log(r["pval"][ok])))}


def both_references(codes, P, R, Wt, H, z_cutoff, penalty, least=1, tol=2.0 ** -30, max_iter=50, cap=20):
    """(long-double reference, flags of the float64 reference, eps) after the conditions on the inputs: the flags of the two are equal, at least `least`
    cells are fitted, no |z| lies within 2^-40 z_cutoff of the cutoff, with penalty == 0 no support margin lies in [2^-31, 2^-29] A, and neither reference
    needs more than cap evaluations"""
    r64, rld = checked_pair(codes, P, R, Wt, H, z_cutoff, penalty, least, tol, max_iter, cap)
    return rld, r64["flag"], max(errors(r64, rld, r64["flag"] == 1).values())


def checked_pair(codes, P, R, Wt, H, z_cutoff, penalty, least, tol, max_iter, cap, tol_ld=TOL_LD, t64=None, tld=None):
    """(float64 reference, long-double reference) of both_references after its conditions, read-only; t64, tld: lists for the traces of the two.  A cutoff of
    0 has no neighbourhood: |z| < 0 holds for no finite z, however it was rounded"""
    r64 = firth_reference(codes, P, R, Wt, H, z_cutoff, penalty, tol, max_iter, np.float64, t64)
    rld = firth_reference(codes, P, R, Wt, H, z_cutoff, penalty, tol_ld, 200, LD, tld)
    assert np.array_equal(r64["flag"], rld["flag"]), np.argwhere(r64["flag"] != rld["flag"])[:5]
    assert (r64["flag"] == 1).sum() >= least, np.bincount(r64["flag"].ravel())
    fin = np.isfinite(r64["z"])
    assert z_cutoff == 0 or not np.any(np.abs(np.abs(r64["z"][fin]) - z_cutoff) <= 2.0 ** -40 * z_cutoff)
    if penalty == 0:
        m = np.array(rld["margins"])
        assert not np.any((m >= 2.0 ** -31) & (m <= 2.0 ** -29))
    assert max(r64["evals"].max(), rld["evals"].max()) <= cap, (r64["evals"].max(), rld["evals"].max())
    for v in list(rld.values()) + list(r64.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r64, rld


def penalised_loglik(beta, g, p, y, penalty):
    """(l*(beta), the sum of the absolute values of its terms) in the type of g"""
    eta = np.log(p / (1 - p)) + beta * g
    lp, lq = -np.logaddexp(0, -eta), -np.logaddexp(0, eta)           # log pi, log(1 - pi)
    terms = np.where(y > 0, lp, lq)
    pi = np.exp(lp)
    pen = 0.5 * np.log((g * g * pi * (1 - pi)).sum()) if penalty else 0 * beta
    return terms.sum() + pen, np.abs(terms).sum() + abs(pen)


# ---- tests/test_assoc_firth_limits_{cpu,gpu}.py: the trace of the Newton loop, the error measures with beta^ = 0, and the cases, each built once per process
# and read-only.  A trace is a list with one dict per fitted item, in the order of the fits ((trait, SNP) ascending): cell = (s, c), U, margin (/ A), status
# (OUTSIDE: the support test ended it before an evaluation), evals, chisq (before max(0, .); None unless solved) and, per evaluation, the lists
#   beta      where f and f' were evaluated
#   replaced  penalty == 1 and the penalised slope `alt` was not positive, so K'' stood in for it
#   ratio     alt / K'' (NaN without the penalty)
#   bisected  beta' was not strictly inside the bracket and the middle replaced it (False where the loop ended before that decision)
#   edge      the distance of the Newton beta' to the bracket end it can fall behind, over |beta'|, before that decision (NaN where the loop ended before it; inf
#             where that end is infinite).  One end of the bracket is beta itself (the sign of f has just moved it there), and beta' = beta - f / f' with f' > 0
#             lies on its inner side by the step, which the stop rule has just found above tol |beta'|: that distance is between tol and 2^-20 on the last
#             step but one of nearly every converging item and decides nothing.  `edge` is the distance to the OTHER end: hi if f < 0, else lo
#   reach     max |beta g_i| over the individuals with g_i != 0
def limit_errors(got, ref, cells, tail=False):
    """errors() for cases that hold beta^ = 0 and p-values below FLOOR: where the reference's |beta| < 2^-20 se the difference in beta is taken over se, not
    over |beta|; a reference chisq of exactly 0 requires 0 <= chisq of got (its size is bounded like every other: |d chisq| / max(1, chisq)); tail: log pval is
    left to tail_errors of tests/_assoc_spa_ref.py and is not among the measures"""
    def over(v):
        return float(v.max()) if v.size else 0.0
    g = {k: np.asarray(got[k])[cells].astype(LD) for k in ("beta", "se", "chisq", "pval")}
    r = {k: np.asarray(ref[k])[cells].astype(LD) for k in ("beta", "se", "chisq", "pval")}
    small = np.abs(r["beta"]) < 2.0 ** -20 * r["se"]
    assert np.all(g["chisq"][r["chisq"] == 0] >= 0)
    out = {"beta": over(np.abs(g["beta"] - r["beta"]) / np.where(small, r["se"], np.abs(r["beta"]))), "se": over(np.abs(g["se"] - r["se"]) / r["se"]),
           "chisq": over(np.abs(g["chisq"] - r["chisq"]) / np.maximum(1, r["chisq"]))}
    if not tail:
        ok = r["pval"] > FLOOR
        assert np.all(g["pval"][ok] > 0)
        out["pval"] = over(np.abs(np.log(g["pval"][ok]) - np.log(r["pval"][ok])))
    return out


def limits_references(codes, P, R, Wt, H, z_cutoff, penalty, least=1, tol=2.0 ** -30, max_iter=50, cap=20, tol_ld=TOL_LD, tail=False):
    """both_references with the traces: dict(rld, r64, flags, eps, t64, tld); eps by limit_errors"""
    t64, tld = [], []
    r64, rld = checked_pair(codes, P, R, Wt, H, z_cutoff, penalty, least, tol, max_iter, cap, tol_ld, t64, tld)
    assert [t["cell"] for t in t64] == [t["cell"] for t in tld]
    return dict(rld=rld, r64=r64, flags=r64["flag"], eps=max(limit_errors(r64, rld, r64["flag"] == 1, tail).values()), t64=t64, tld=tld)


LIMITS_INDIV = (259, 1027)
#               TAIL_ROWS' fields (fraction of the cases, their allele count, controls at the count 1), then flip: the row is 2 - that pattern, which puts the
#               allele into nearly all controls and U on the negative side
BISECT_ROWS = ([r + (False,) for r in TAIL_ROWS] + [(1.0, 1, 1, False), (1.0, 1, 2, False), (1.0, 1, 5, False), (0.9, 1, 1, False), (0.9, 1, 2, False), (0.8, 1, 1, False),
                                                   (0.75, 1, 2, False), (0.6, 1, 1, False)] + [r + (True,) for r in TAIL_ROWS] + [(1.0, 1, 2, True), (0.9, 1, 1, True)])
BISECT_SNPS, BISECT_CUTOFF = 33, 1.0


@functools.lru_cache(maxsize=None)
def bisect_operands(indiv, kh=1):
    """limits_operands(indiv, 33, 1, kh) with BISECT_ROWS written over the first rows as tail_operands writes TAIL_ROWS: no missing call"""
    codes, _, Y, W, P, R, Wt, H = limits_operands(indiv, BISECT_SNPS, 1, kh)
    codes = codes.copy()
    cases, controls = np.flatnonzero(Y[:, 0] > 0), np.flatnonzero(Y[:, 0] == 0)
    rng = np.random.default_rng([LIMITS_SEED, indiv, kh, 7])
    for row, (fraction, count, at_one, flip) in enumerate(BISECT_ROWS):
        codes[row] = 0
        codes[row, cases[:int(round(fraction * len(cases)))]] = count
        codes[row, rng.choice(controls, at_one, replace=False)] = 1
        if flip:
            codes[row] = 2 - codes[row]
    return frozen(codes, pack(codes)) + (Y, W, P, R, Wt, H)


def made_operands(codes, Y, P, Wt=None):
    """(codes, packed rows, Y, None, P, R, Wt, H) with kh = 0 and probabilities made by the caller: R = Y - P, Wt = P (1 - P) unless given, H without a column"""
    Y, P = np.asfortranarray(Y, dtype=np.float64), np.asfortranarray(P, dtype=np.float64)
    Wt = np.asfortranarray(P * (1 - P) if Wt is None else Wt)
    codes = np.ascontiguousarray(codes, dtype=np.int8)
    return frozen(codes, pack(codes), Y, None, P, np.asfortranarray(Y - P), Wt, np.zeros((Y.shape[0], 0), order="F"))


def _ordinary(rng, snps, indiv, maf, keep_out=0):
    """rows of binomial(2, maf) allele counts with 5 % missing calls; the first keep_out individuals carry nothing"""
    codes = rng.binomial(2, maf, (snps, indiv)).astype(np.int8)
    codes[rng.random((snps, indiv)) < 0.05] = -1
    codes[:, :keep_out] = 0
    return codes


ALT_SNPS, ALT_CUTOFF = 24, 1.0
#           carriers at 1, carriers at 2; the first carrier at 1 and the first at 2 are cases, no one else who carries
ALT_ROWS = [(4, 1), (5, 1), (3, 1), (6, 1), (2, 1), (4, 2)]


@functools.lru_cache(maxsize=None)
def alt_operands(indiv):
    """kh = 0, P = 0.01 everywhere, 6 % cases; the rows of ALT_ROWS (no missing call), then ordinary rows at MAF 0.15"""
    rng = np.random.default_rng([LIMITS_SEED, indiv, 21])
    y = (rng.random(indiv) < 0.06).astype(np.float64)
    y[:4] = (1, 1, 0, 0)
    codes = _ordinary(rng, ALT_SNPS, indiv, 0.15)
    cases, controls = np.flatnonzero(y > 0), np.flatnonzero(y == 0)
    for row, (ones, twos) in enumerate(ALT_ROWS):
        codes[row] = 0
        codes[row, np.roll(controls, -7 * row)[:ones + twos - 2]] = [1] * (ones - 1) + [2] * (twos - 1)
        codes[row, np.roll(cases, -row)[:2]] = (1, 2)
    return made_operands(codes, y[:, None], np.full((indiv, 1), 0.01))


NEG_SNPS, NEG_CUTOFF = 24, 1.0


@functools.lru_cache(maxsize=None)
def negative_operands(indiv):
    """kh = 0, P = 0.05 everywhere, 8 % cases, U < 0 on the first nine rows (no missing call): rows 0-2 carried by 30, 45 and 60 controls alone (the edge of
    the support on the negative side), rows 3-5 by nearly all controls at 2 and one case at 1 (margin / A = 1 / (alleles)), rows 6-8 by 120-200 controls and two
    cases; then ordinary rows at MAF 0.15"""
    rng = np.random.default_rng([LIMITS_SEED, indiv, 22])
    y = (rng.random(indiv) < 0.08).astype(np.float64)
    y[:4] = (1, 1, 0, 0)
    codes = _ordinary(rng, NEG_SNPS, indiv, 0.15)
    cases, controls = np.flatnonzero(y > 0), np.flatnonzero(y == 0)
    codes[:9] = 0
    for row, m in enumerate((30, 45, 60)):
        codes[row, rng.choice(controls, m, replace=False)] = 1 + row % 2
    for row, m in zip((3, 4, 5), (len(controls), len(controls) - 40, len(controls) // 2 + 60)):
        codes[row, controls[:m]] = 2
        codes[row, cases[row]] = 1
    for row, m in zip((6, 7, 8), (120, 160, 200)):
        codes[row, rng.choice(controls, m, replace=False)] = 1
        codes[row, cases[:2]] = 1
    return made_operands(codes, y[:, None], np.full((indiv, 1), 0.05))


SAT_SNPS, SAT_CUTOFF = 24, 1.0
#           zone of twenty individuals each: the fitted probability there, and y of its first two / its other individuals
SAT_ZONES = [(1e-5, 1, 0), (1e-7, 1, 0), (1 - 1e-5, 0, 1), (1 - 1e-7, 0, 1), (0.0, 1, 0), (1.0, 0, 1)]
SAT_KEEP_OUT = 20 * len(SAT_ZONES)


@functools.lru_cache(maxsize=None)
def saturated_operands(indiv):
    """kh = 0; six zones of twenty individuals by SAT_ZONES (with p in {0, 1} the weight is made 0.0475, so that V > 0 and z is finite while K''(0) = 0), P = 0.05
    behind them with 8 % cases.  Rows 2 z and 2 z + 1 (z < 6, no missing call) are carried by five and by seven individuals of zone z alone, the zone's first
    two among them: U > 0 in the zones of small p, U < 0 in those of large p, and never on the edge of the support.  Then ordinary rows at MAF 0.15 that no one
    of the zones carries"""
    rng = np.random.default_rng([LIMITS_SEED, indiv, 23])
    y = (rng.random(indiv) < 0.08).astype(np.float64)
    p, w = np.full(indiv, 0.05), np.full(indiv, 0.0475)
    codes = _ordinary(rng, SAT_SNPS, indiv, 0.15, SAT_KEEP_OUT)
    codes[:2 * len(SAT_ZONES)] = 0
    for z, (prob, first, others) in enumerate(SAT_ZONES):
        at = slice(20 * z, 20 * z + 20)
        p[at] = prob
        if 0 < prob < 1:
            w[at] = prob * (1 - prob)
        y[at] = others
        y[20 * z:20 * z + 2] = first
        codes[2 * z, 20 * z:20 * z + 5] = 1
        codes[2 * z + 1, 20 * z:20 * z + 7] = (1, 2, 1, 1, 2, 1, 1)
    return made_operands(codes, y[:, None], p[:, None], w[:, None])


ZERO_SNPS = 33
ZERO_CASES = [(67, 1), (259, 3)]            # indiv, n


@functools.lru_cache(maxsize=None)
def zero_operands(indiv, n):
    """kh = 0, P = 0.5 everywhere, half of every trait's individuals cases.  Row 0 entirely missing, row 1 monomorphic (flag 3 both); rows 2-10: no missing
    call, as many case as control carriers of trait (row % n) at each allele count, so that its U is a sum of +-1/2 and +-1 that cancels exactly; rows 11-16: the
    same with one missing call (U = +-mu / 2, |z| < 0.05); then ordinary rows at MAF 0.3"""
    rng = np.random.default_rng([LIMITS_SEED, indiv, n, 24])
    Y = np.zeros((indiv, n))
    for c in range(n):
        Y[rng.permutation(indiv)[:indiv // 2], c] = 1
    codes = _ordinary(rng, ZERO_SNPS, indiv, 0.3)
    codes[0] = -1
    codes[1:17] = 0
    for row in range(2, 17):
        c = row % n
        cases, controls = rng.permutation(np.flatnonzero(Y[:, c] > 0)), rng.permutation(np.flatnonzero(Y[:, c] == 0))
        ones, twos = 1 + row % 3, row % 2
        for who in (cases, controls):
            codes[row, who[:ones]] = 1
            codes[row, who[ones:ones + twos]] = 2
        if row >= 11:
            codes[row, cases[ones + twos]] = -1
    return made_operands(codes, Y, np.full((indiv, n), 0.5))


LIMITS_TAIL_INDIV = (1027, 4099, 8195)
#                 on bisect_operands(259): a cutoff below the ordinary rows' |z| and a tolerance at which some of them stop after two evaluations, while the rows
#                 of BISECT_ROWS, whose first step overshoots, still run out of six
MAX_ITER_CUTOFF, MAX_ITER_TOL, MAX_ITERS = 0.25, 2.0 ** -6, (2, 4, 6)
LIMITS_TOLS = (2.0 ** -12, 2.0 ** -40)


def limits_case(kind, *key):
    """(operands, z_cutoff, tail) of a case of the limits tests: ("bisect", indiv, kh), ("alt", indiv), ("negative", indiv), ("saturated", indiv),
    ("zero", indiv, n), ("tail", indiv), ("list", index into LIST_CASES)"""
    if kind == "bisect":
        return bisect_operands(*key), BISECT_CUTOFF, False
    if kind == "alt":
        return alt_operands(*key), ALT_CUTOFF, False
    if kind == "negative":
        return negative_operands(*key), NEG_CUTOFF, False
    if kind == "saturated":
        return saturated_operands(*key), SAT_CUTOFF, False
    if kind == "zero":
        return zero_operands(*key), 0.0, False
    if kind == "tail":
        return tail_operands(*key), 1.0, True
    indiv, snps, n, kh, z_cutoff = LIST_CASES[key[0]]
    return limits_operands(indiv, snps, n, kh), z_cutoff, False


@functools.lru_cache(maxsize=None)
def limits_reference(kind, key, penalty, tol=2.0 ** -30, tol_ld=TOL_LD, z_cutoff=None):
    """limits_references of limits_case(kind, *key), once per process"""
    (codes, _, _, _, P, R, Wt, H), cutoff, tail = limits_case(kind, *key)
    return limits_references(codes, P, R, Wt, H, cutoff if z_cutoff is None else z_cutoff, penalty, 1, tol, 50, 20, tol_ld, tail)


@functools.lru_cache(maxsize=None)
def max_iter_flags(penalty, max_iter, T=np.float64, factor=1.0):
    """(flags, trace) of bisect_operands(259) at MAX_ITER_CUTOFF, factor MAX_ITER_TOL and max_iter evaluations in the type T"""
    codes, _, _, _, P, R, Wt, H = bisect_operands(259)
    trace = []
    flags = firth_reference(codes, P, R, Wt, H, MAX_ITER_CUTOFF, penalty, factor * MAX_ITER_TOL, max_iter, T, trace)["flag"]
    flags.setflags(write=False)
    return flags, trace
