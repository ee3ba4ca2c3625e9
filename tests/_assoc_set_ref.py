"""References of the set-test tests (mxa_assoc_set / mxa_assoc_skat_pvalue).  numpy, math and mpmath only; nothing of the library is imported.

set_reference   the definition of the header from the raw codes, in np.longdouble (the sums over the individuals sorted by magnitude) or in plain float64 numpy
                (dtype=np.float64): mu, U, a, S, Phi and the six statistics of every (set, trait), and for each value the SCALE its error is measured by.
                The evaluation runs over the DISTINCT SNPs of a set (a set of 1024 entries drawn from 64 SNPs costs 64 x 64 sums): with s_u = the sum of omega
                and g_u = the sum of omega^2 over the entries of SNP u, varB = sum_uv s_u s_v Phi_uv, c1 = sum_u g_u Phi_uu, c2 = sum_uv g_u g_v Phi_uv^2 and
                c4 = sum_uv g_u g_v ((Phi G Phi)_uv)^2 with G = diag(g) -- the same numbers as the sums over the entries, by another route.
scales          "the sum of the absolute values of its terms", each term taken down to the individuals (first-order propagation):
                  U_j: sU = sum_i |x r|;  Phi_jj': sPhi = sum_i w |x_j x_j'| + sum_h |a_jh a_j'h|;
                  B: sum_j |omega_j| sU_j;  Q: Q + sum_j 2 |u_j| |omega_j| sU_j  (u = omega U);
                  varB: sum |s_u s_v| sPhi_uv;  c1: sum g_u sPhi_uu;  c2: c2 + sum g_u g_v 2 |Phi_uv| sPhi_uv;
                  c4: c4 + sum g_u g_v 2 |T_uv| sT_uv with T = Phi G Phi, sT_uv = sum_t g_t (|Phi_ut| sPhi_tv + sPhi_ut |Phi_tv| + |Phi_ut Phi_tv|).
                These scales are larger than the literal last sum of a statistic (sum |omega U| for B, Q itself, sum |A|, sum |A_jj|, c2, c4), because U and Phi
                carry errors relative to THEIR terms, not to themselves: over the cases of tests/test_assoc_set_gpu.py by a factor of (median / largest) 11.5 / 342
                (B), 18.5 / 685 (Q), 1.0 / 3.5 (varB), 1.0 / 3.6 (c1), 3.0 / 7.0 (c2), 7.0 / 17 (c4).
scaled_error    max |got - ref| / scale (where the scale is zero the two must agree exactly)
upper_gamma     Q(l / 2, x / 2) by mpmath at 50 digits
random_case     codes, R, Wt, H for the accuracy tests (the identities are algebraic: no null model needs to have been fitted)
simulate        the calibration study: genes of rare variants under a Gaussian or a balanced logistic null
"""
import numpy as np

from _assoc_ref import LD, genotypes, pack  # noqa: F401

TILE = 16            # the Gram tile edge of k_assoc_set_gram
SPLIT = 4096         # individuals of one piece of its split
TOL = 2.0 ** -48


def _ssum(t, dtype):
    """sum over the last axis; long double: the terms sorted by magnitude first"""
    if dtype is LD:
        t = np.take_along_axis(t, np.argsort(np.abs(t), axis=-1), -1)
    return t.sum(-1)


def imputed(codes, dtype):
    codes = np.asarray(codes)
    z = np.where(codes < 0, 0, codes).astype(dtype)
    with np.errstate(all="ignore"):
        mu = z.sum(1).astype(dtype) / (codes >= 0).sum(1).astype(dtype)
    return np.where(codes < 0, mu[:, None], z)


def set_reference(codes, R, Wt, H, sets, weights=None, dtype=LD):
    """per set a dict: phi, sphi (n, m, m); stat, sstat (n, 6) in the order B, varB, Q, c1, c2, c4; U, sU (n, m)"""
    codes = np.asarray(codes)
    R, Wt = np.asarray(R).reshape(codes.shape[1], -1), np.asarray(Wt).reshape(codes.shape[1], -1)
    n = R.shape[1]
    H = np.zeros((codes.shape[1], 0)) if H is None else np.asarray(H)
    kh = H.shape[1] // n
    out = []
    for k, idx in enumerate(sets):
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        m = idx.size
        om = np.ones(m, dtype) if weights is None else np.asarray(weights[k]).astype(dtype)
        uniq, inv = np.unique(idx, return_inverse=True)
        u = uniq.size
        x = imputed(codes[uniq], dtype).reshape(u, codes.shape[1])
        s1, sa, g = (np.zeros(u, dtype) for _ in range(3))
        np.add.at(s1, inv, om)
        np.add.at(sa, inv, np.abs(om))
        np.add.at(g, inv, om * om)
        res = dict(phi=np.zeros((n, m, m), dtype), sphi=np.zeros((n, m, m), dtype), stat=np.zeros((n, 6), dtype), sstat=np.zeros((n, 6), dtype),
                   U=np.zeros((n, m), dtype), sU=np.zeros((n, m), dtype))
        with np.errstate(all="ignore"):
            for c in range(n):
                r, w = R[:, c].astype(dtype), Wt[:, c].astype(dtype)
                U, sU = _ssum(x * r, dtype), _ssum(np.abs(x * r), dtype)
                xx = x[:, None, :] * x[None, :, :] * w
                phi, sphi = _ssum(xx, dtype), _ssum(np.abs(xx), dtype)
                for h in range(kh):
                    a = _ssum(x * H[:, c * kh + h].astype(dtype), dtype)
                    phi = phi - a[:, None] * a[None, :]
                    sphi = sphi + np.abs(a[:, None] * a[None, :])
                uj = om * U[inv]
                gg, ss = g[:, None] * g[None, :], sa[:, None] * sa[None, :]
                T = (phi * g[None, :]) @ phi
                sT = (np.abs(phi) * g[None, :]) @ sphi + (sphi * g[None, :]) @ np.abs(phi) + (np.abs(phi) * g[None, :]) @ np.abs(phi)
                c2, c4 = (gg * phi * phi).sum(), (gg * T * T).sum()
                res["stat"][c] = [uj.sum(), (s1[:, None] * s1[None, :] * phi).sum(), (uj * uj).sum(), (g * np.diagonal(phi)).sum(), c2, c4]
                res["sstat"][c] = [(np.abs(om) * sU[inv]).sum(), (ss * sphi).sum(), (uj * uj).sum() + (2 * np.abs(uj) * np.abs(om) * sU[inv]).sum(),
                                   (g * np.diagonal(sphi)).sum(), c2 + (gg * 2 * np.abs(phi) * sphi).sum(), c4 + (gg * 2 * np.abs(T) * sT).sum()]
                res["phi"][c], res["sphi"][c] = phi[np.ix_(inv, inv)], sphi[np.ix_(inv, inv)]
                res["U"][c], res["sU"][c] = U[inv], sU[inv]
        out.append(res)
    return out


def scaled_error(got, ref, scale):
    got, ref, scale = np.asarray(got).astype(LD), np.asarray(ref).astype(LD), np.asarray(scale).astype(LD)
    if got.size == 0:
        return 0.0
    zero = scale == 0
    assert np.array_equal(got[zero], ref[zero]), "values without any term must be exactly zero"
    if np.all(zero):
        return 0.0
    return float((np.abs(got - ref)[~zero] / scale[~zero]).max())


def upper_gamma(l, x):
    """Q(l / 2, x / 2) as an mpmath number, 50 digits"""
    import mpmath
    with mpmath.workdps(50):
        return +mpmath.gammainc(mpmath.mpf(l) / 2, mpmath.mpf(x) / 2, mpmath.inf, regularized=True)


def random_case(indiv, snps, n, kh, seed, missing=0.05):
    """codes (`missing` missing calls, no edge patterns), R (indiv, n), Wt (indiv, n) in (0.05, 0.25), H (indiv, n kh), Fortran-ordered float64"""
    rng = np.random.default_rng([seed, indiv, snps, n, kh, 19])
    codes = genotypes(snps, indiv, seed, missing=missing, special=False)
    if missing > 0:                                   # no SNP without a called individual here
        codes[:, 0] = np.where(codes[:, 0] < 0, 1, codes[:, 0])
    R = np.asfortranarray(rng.standard_normal((indiv, n)))
    Wt = np.asfortranarray(rng.uniform(0.05, 0.25, (indiv, n)))
    H = np.asfortranarray(rng.standard_normal((indiv, n * kh)) / np.sqrt(4.0 * indiv))
    return codes, R, Wt, H


def pack_dirty(codes, seed):
    """pack(codes) with the padding fields of every row's last byte set to random bits"""
    X = pack(codes).copy()
    indiv = np.asarray(codes).shape[1]
    if indiv % 4:
        keep = (1 << (2 * (indiv % 4))) - 1
        rng = np.random.default_rng([seed, 5])
        X[:, -1] = (X[:, -1] & keep) | (rng.integers(0, 256, X.shape[0]).astype(np.uint8) & np.uint8(255 ^ keep))
    return X


def simulate(seed, indiv=1500, nsets=400, m=8, binary=False):
    """The calibration study: codes (nsets m SNPs, MAF uniform in 0.01-0.05, 2 % missing calls), R, Wt, H of the null model with two covariates (Gaussian:
    R = residual / s^2, Wt = 1 / s^2; logistic, balanced: Newton to convergence), H = W C L^-T, and the weights omega = 1 / sqrt(f (1 - f)) per set"""
    rng = np.random.default_rng(seed)
    snps = nsets * m
    maf = rng.uniform(0.01, 0.05, snps)
    X = (rng.random((snps, indiv)) < maf[:, None]).astype(np.int8) + (rng.random((snps, indiv)) < maf[:, None]).astype(np.int8)
    miss = rng.random((snps, indiv)) < 0.02
    C = np.column_stack([np.ones(indiv), rng.standard_normal((indiv, 2))])
    if binary:
        eta = 0.5 * C[:, 1]
        y = (rng.random(indiv) < 1 / (1 + np.exp(-eta))).astype(float)
        gam = np.zeros(3)
        for _ in range(30):
            p = 1 / (1 + np.exp(-C @ gam))
            w = p * (1 - p)
            gam += np.linalg.solve(C.T @ (w[:, None] * C), C.T @ (y - p))
        p = 1 / (1 + np.exp(-C @ gam))
        w, r = p * (1 - p), y - p
    else:
        y = 0.5 * C[:, 1] + rng.standard_normal(indiv)
        b = np.linalg.lstsq(C, y, rcond=None)[0]
        res = y - C @ b
        s2 = res @ res / (indiv - 3)
        r, w = res / s2, np.full(indiv, 1 / s2)
    L = np.linalg.cholesky(C.T @ (w[:, None] * C))
    H = (w[:, None] * C) @ np.linalg.inv(L).T
    codes = np.where(miss, -1, X).astype(np.int8)
    om = 1 / np.sqrt(maf * (1 - maf))
    sets = [np.arange(k * m, (k + 1) * m) for k in range(nsets)]
    return codes, np.asfortranarray(r.reshape(-1, 1)), np.asfortranarray(w.reshape(-1, 1)), np.asfortranarray(H), sets, [om[s] for s in sets]
