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
"""
import numpy as np

from _assoc_score_ref import score_sums
from _assoc_spa_ref import FAILED, LD, OUTSIDE, SOLVED, TOL_LD, erfc_of, cgf, normal_p  # noqa: F401

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


def fit(g, p, U, penalty, tol, max_iter, T):
    c0, A = (g * p).sum(), np.abs(g).sum()
    sigma = 1 if U >= 0 else -1             # (the margin is reported for both penalties; only penalty == 0 acts on it)
    b = (np.maximum(g, 0).sum() if sigma > 0 else np.minimum(g, 0).sum()) - c0
    margin = T(sigma) * (b - U)
    rel = float(margin / A) if A > 0 else 0.0
    if penalty == 0 and margin <= T(2.0 ** -30) * A:
        return OUTSIDE, None, None, None, None, 0, rel
    beta, lo, hi, hat, evals, k20 = T(0), T(-np.inf), T(np.inf), None, 0, None
    with np.errstate(all="ignore"):
        while evals < max_iter:
            K1, K2, K3, K4 = cgf4(beta, g, p, c0)
            evals += 1
            if evals == 1:
                k20 = K2
            f, fp = K1 - U, K2
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
            if not np.isfinite(bn):
                return FAILED, None, None, None, None, evals, rel
            if abs(bn - beta) <= T(tol) * abs(bn):
                hat = bn
                break
            if not (lo < bn < hi):
                bn = (lo + hi) / 2
                if not np.isfinite(bn):
                    return FAILED, None, None, None, None, evals, rel
            beta = bn
        if hat is None:
            return FAILED, None, None, None, None, evals, rel
        K, _, K2 = cgf(hat, g, p, c0)
    return SOLVED, hat, K, K2, k20, evals, rel


def one_step(U, V, z, T):
    with np.errstate(all="ignore"):
        return U / V, 1 / np.sqrt(V), z * z, normal_p(z, T)


def results_of_fit(res, U, V, z, penalty, T):
    """(flag, beta, se, chisq, pval) from fit's result"""
    status, hat, K, K2, k20 = res[:5]
    if status == SOLVED:
        with np.errstate(all="ignore"):
            se = 1 / np.sqrt(K2)
            x2 = 2 * (hat * U - K)
            if penalty:
                x2 = x2 + np.log(K2 / k20)
        if np.isfinite(se) and np.isfinite(x2):
            x2 = max(x2, T(0))
            return 1, hat, se, x2, erfc_of(np.sqrt(x2 / 2), T)
    return (2,) + one_step(U, V, z, T)


def firth_item(x, p, tau, a, U, V, z, penalty, tol, max_iter, T):
    """(flag, beta, se, chisq, pval, evaluations, support margin / A) of one item that is to be fitted.  x: the allele counts with mu at the missing calls,
    tau: (kh, indiv) = h / w, a: (kh,)"""
    g = x.astype(T).copy()
    for j in range(len(a)):
        g = g - a[j] * tau[j]
    res = fit(g, p, U, penalty, tol, max_iter, T)
    return results_of_fit(res, U, V, z, penalty, T) + (res[5], res[6])


def firth_reference(codes, P, R, Wt, H, z_cutoff=2.0, penalty=1, tol=2.0 ** -30, max_iter=50, T=np.float64):
    """dict of beta, se, chisq, pval, z (snps, n) in T, flag and evals (snps, n) int32, and margins: the support margins / A of the fitted items"""
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
                    got = firth_item(x, Pt[:, c], tau, a, U, V, z, penalty, tol, max_iter, T)
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
    r64 = firth_reference(codes, P, R, Wt, H, z_cutoff, penalty, tol, max_iter, np.float64)
    rld = firth_reference(codes, P, R, Wt, H, z_cutoff, penalty, TOL_LD, 200, LD)
    assert np.array_equal(r64["flag"], rld["flag"]), np.argwhere(r64["flag"] != rld["flag"])[:5]
    assert (r64["flag"] == 1).sum() >= least, np.bincount(r64["flag"].ravel())
    fin = np.isfinite(r64["z"])
    assert not np.any(np.abs(np.abs(r64["z"][fin]) - z_cutoff) <= 2.0 ** -40 * z_cutoff)
    if penalty == 0:
        m = np.array(rld["margins"])
        assert not np.any((m >= 2.0 ** -31) & (m <= 2.0 ** -29))
    assert max(r64["evals"].max(), rld["evals"].max()) <= cap, (r64["evals"].max(), rld["evals"].max())
    eps = max(errors(r64, rld, r64["flag"] == 1).values())
    for v in list(rld.values()) + [r64["flag"]]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return rld, r64["flag"], eps


def penalised_loglik(beta, g, p, y, penalty):
    """(l*(beta), the sum of the absolute values of its terms) in the type of g"""
    eta = np.log(p / (1 - p)) + beta * g
    lp, lq = -np.logaddexp(0, -eta), -np.logaddexp(0, eta)           # log pi, log(1 - pi)
    terms = np.where(y > 0, lp, lq)
    pi = np.exp(lp)
    pen = 0.5 * np.log((g * g * pi * (1 - pi)).sum()) if penalty else 0 * beta
    return terms.sum() + pen, np.abs(terms).sum() + abs(pen)
