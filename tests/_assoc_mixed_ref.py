"""Dense references of the mixed-model association tests (miraculix_amd/mixed.py).  numpy, and torch's CPU generator for the seeded draws; nothing of the
library is imported.  float64 throughout; K is formed, and np.linalg.solve stands where the library runs conjugate gradients.

pack / unpack          PLINK rows from codes (snps, indiv) in {-1 (missing), 0, 1, 2} and back
kinship_dense          K = sum_b Zc_b^T Zc_b / sum_b s_b with Zc = z - 2 f, a missing call as z = 0 BEFORE centring (it contributes -2 f)
gram_schmidt_twice     the orthonormal basis Qc of C = [1 | W]
rademacher, picks      the seeded probes and calibration SNPs, by the recipe the library documents
he_estimate            randomized Haseman-Elston for given probes; he_exact: the same with exact traces
null_ref               the GLS fit for given h2: gamma, r = P y, sigma2, P itself
block_cg               the library's block CG recurrence in numpy (iteration counts)
mixed_ref              the whole scan; ols_ref: the plain score test without K; lambda_gc
structured_case        two Balding-Nichols sub-populations crossed with sib-ships of 4: the data of the inflation test
"""
import numpy as np


def pack(codes):
    """(snps, ceil(indiv / 4)) uint8: 0 -> 00, missing -> 01, 1 -> 10, 2 -> 11, four per byte, low bits first, padding fields 00"""
    codes = np.asarray(codes)
    snps, indiv = codes.shape
    field = np.where(codes < 0, 1, np.where(codes == 0, 0, codes + 1)).astype(np.uint8)
    pad = (-indiv) % 4
    if pad:
        field = np.concatenate([field, np.zeros((snps, pad), np.uint8)], axis=1)
    c4 = field.reshape(snps, -1, 4)
    return np.ascontiguousarray(c4[:, :, 0] | (c4[:, :, 1] << 2) | (c4[:, :, 2] << 4) | (c4[:, :, 3] << 6)).astype(np.uint8)


def unpack(plink, indiv):
    p = np.asarray(plink, dtype=np.uint8)
    field = np.stack([(p >> (2 * q)) & 3 for q in range(4)], axis=2).reshape(p.shape[0], -1)[:, :indiv].astype(np.int64)
    return np.where(field == 1, -1, np.where(field == 0, 0, field - 1))


def random_codes(snps, indiv, seed, missing=0.0):
    rng = np.random.default_rng([seed, snps, indiv, 11])
    p = rng.uniform(0.1, 0.6, snps)
    codes = rng.binomial(2, p[:, None], (snps, indiv)).astype(np.int64)
    if missing > 0:
        codes[rng.random((snps, indiv)) < missing] = -1
    return codes


def block_list(bounds, leave_out=None):
    return [b for b in range(len(bounds) - 1) if b != leave_out]


def kinship_dense(codes, bounds, leave_out=None):
    """K (indiv, indiv): the blocks are added in ascending order, as the operator adds them"""
    codes = np.asarray(codes)
    snps, indiv = codes.shape
    z = np.where(codes < 0, 0, codes).astype(np.float64)
    f = z.sum(1) / (2.0 * indiv)
    Zc = z - 2.0 * f[:, None]                                  # a missing call: 0 - 2 f
    K, s = np.zeros((indiv, indiv)), 0.0
    for b in block_list(bounds, leave_out):
        b0, b1 = bounds[b], bounds[b + 1]
        K += Zc[b0:b1].T @ Zc[b0:b1]
        s += float(2.0 * np.sum(f[b0:b1] * (1.0 - f[b0:b1])))
    return K / s


def gram_schmidt_twice(C):
    C = np.asarray(C, dtype=np.float64)
    Q = np.zeros(C.shape)
    for j in range(C.shape[1]):
        v = C[:, j].copy()
        for _ in range(2):
            for p in range(j):
                v -= (Q[:, p] @ v) * Q[:, p]
        Q[:, j] = v / np.sqrt(v @ v)
    return Q


def design(indiv, W):
    C = np.ones((indiv, 1)) if W is None or np.asarray(W).size == 0 else np.concatenate([np.ones((indiv, 1)), np.asarray(W, np.float64).reshape(indiv, -1)], axis=1)
    return C, gram_schmidt_twice(C)


def rademacher(indiv, probes, seed):
    import torch
    g = torch.Generator().manual_seed(int(seed))
    return (torch.randint(0, 2, (int(probes), int(indiv)), generator=g, dtype=torch.int64).to(torch.float64) * 2.0 - 1.0).numpy().T.copy()


def picks(size, count, seed, unit):
    import torch
    g = torch.Generator().manual_seed(int(seed) + 7919 * (int(unit) + 1))
    return np.sort(torch.randperm(int(size), generator=g)[:min(int(count), int(size))].numpy())


def hadamard(m):
    H = np.ones((1, 1))
    while H.shape[0] < m:
        H = np.block([[H, H], [H, -H]])
    return H


def _he_solve(t1, t2, dof, quad, yy):
    det = t2 * dof - t1 * t1
    sg2 = (dof * quad - t1 * yy) / det
    se2 = (t2 * yy - t1 * quad) / det
    return np.clip(sg2 / (sg2 + se2), 0.0, 0.999)


def he_estimate(K, Y, Qc, Z):
    """h2 (n,) for the probes Z (indiv, probes)"""
    M = np.eye(K.shape[0]) - Qc @ Qc.T
    Kt = M @ K @ M
    Yt = M @ Y
    KZ = Kt @ Z
    t1, t2 = np.mean(np.sum(Z * KZ, 0)), np.mean(np.sum(KZ * KZ, 0))
    return _he_solve(t1, t2, float(K.shape[0] - Qc.shape[1]), np.sum(Yt * (Kt @ Yt), 0), np.sum(Yt * Yt, 0))


def he_exact(K, Y, Qc):
    """the same with t1 = tr K~ and t2 = tr K~^2"""
    M = np.eye(K.shape[0]) - Qc @ Qc.T
    Kt = M @ K @ M
    Yt = M @ Y
    return _he_solve(np.trace(Kt), np.sum(Kt * Kt), float(K.shape[0] - Qc.shape[1]), np.sum(Yt * (Kt @ Yt), 0), np.sum(Yt * Yt, 0))


def null_ref(K, Y, C, h2):
    """per trait c: dict(tau, gamma, r, sigma2, P, VinvC, G, kappa = 1 + tau lambda_max(K))"""
    indiv = K.shape[0]
    lam_max = float(np.linalg.eigvalsh(K)[-1])
    out = []
    for c in range(Y.shape[1]):
        tau = h2[c] / (1.0 - h2[c])
        V = tau * K + np.eye(indiv)
        Vinv = np.linalg.solve(V, np.eye(indiv))
        Vinv = 0.5 * (Vinv + Vinv.T)
        VinvC = Vinv @ C
        G = C.T @ VinvC
        P = Vinv - VinvC @ np.linalg.solve(G, VinvC.T)
        gamma = np.linalg.solve(G, VinvC.T @ Y[:, c])
        r = Vinv @ Y[:, c] - VinvC @ gamma
        out.append(dict(tau=tau, gamma=gamma, r=r, sigma2=float(Y[:, c] @ r) / (indiv - C.shape[1]), P=P, VinvC=VinvC, G=G, kappa=1.0 + tau * lam_max))
    return out


def block_cg(A, B, tol=1e-10, max_iter=500):
    """(X, iters, relres) by the recurrence of mixed.solve"""
    n = B.shape[1]
    X, R = np.zeros_like(B), B.copy()
    P = R.copy()
    rs = np.sum(R * R, 0)
    bnorm = np.sqrt(rs)
    thr = tol * bnorm
    active = bnorm > thr
    iters = np.zeros(n, np.int64)
    for _ in range(max_iter):
        if not active.any():
            break
        AP = A @ P
        with np.errstate(all="ignore"):
            alpha = np.where(active, rs / np.sum(P * AP, 0), 0.0)
            X += P * alpha
            R -= AP * alpha
            rs_new = np.sum(R * R, 0)
            beta = np.where(active, rs_new / rs, 0.0)
        P = R + P * beta
        iters += active
        rs = np.where(active, rs_new, rs)
        active = active & (np.sqrt(rs) > thr)
    with np.errstate(all="ignore"):
        return X, iters, np.where(bnorm > 0, np.sqrt(rs) / bnorm, 0.0)


def imputed(codes):
    """(x (snps, indiv) with missing calls as the SNP's mean over its called individuals, valid (snps,)); a SNP without a called individual or without variance
    is not valid and has a zero row"""
    codes = np.asarray(codes)
    z = np.where(codes < 0, 0, codes).astype(np.float64)
    N = (codes >= 0).sum(1).astype(np.float64)
    Sz, Szz = z.sum(1), (z * z).sum(1)
    valid = (N > 0) & (N * Szz - Sz * Sz > 0)
    with np.errstate(all="ignore"):
        mu = np.where(valid, Sz / N, 0.0)
    return np.where(codes < 0, mu[:, None], z) * valid[:, None], valid


def erfc_vec(a):
    from math import erfc
    return np.array([erfc(v) if np.isfinite(v) else np.nan for v in np.asarray(a).reshape(-1)]).reshape(np.shape(a))


def mixed_ref(codes, bounds, Y, W=None, loco=True, h2=None, calib_snps=200, exact_cutoff=None, seed=1, probes=32):
    """dict(score, var, z, pval, beta, se (snps, n), flag, h2 (n,), gamma (units, n), kappa: the largest 1 + tau lambda_max(K) over the units and traits,
    nulls: per unit the list of null_ref)"""
    codes = np.asarray(codes)
    snps, indiv = codes.shape
    Y = np.asarray(Y, np.float64).reshape(indiv, -1)
    n = Y.shape[1]
    C, Qc = design(indiv, W)
    M = np.eye(indiv) - Qc @ Qc.T
    if h2 is None:
        h2 = he_estimate(kinship_dense(codes, bounds), Y, Qc, rademacher(indiv, probes, seed))
    h2 = np.broadcast_to(np.asarray(h2, np.float64).reshape(-1), (n,)).copy()
    loco = bool(loco) and len(bounds) > 2
    units = [(c, bounds[c], bounds[c + 1]) for c in range(len(bounds) - 1)] if loco else [(None, 0, snps)]
    x_all, valid = imputed(codes)
    score, var, z = (np.full((snps, n), np.nan) for _ in range(3))
    flag = np.zeros((snps, n), np.int32)
    gamma = np.zeros((len(units), n))
    kappa, nulls = 0.0, []
    for u, (leave, b0, b1) in enumerate(units):
        nr = null_ref(kinship_dense(codes, bounds, leave), Y, C, h2)
        nulls.append(nr)
        xu = x_all[b0:b1]
        xc = xu[picks(b1 - b0, calib_snps, seed, u)]
        den = np.sum(xc * (xc @ M))
        xMx = np.sum(xu * (xu @ M), 1)
        for c in range(n):
            kappa = max(kappa, nr[c]["kappa"])
            gamma[u, c] = np.sum(xc * (xc @ nr[c]["P"])) / den
            s2 = nr[c]["sigma2"]
            with np.errstate(all="ignore"):
                U = xu @ nr[c]["r"] / s2
                V = np.where(valid[b0:b1], gamma[u, c] * xMx / s2, np.nan)
                zz = U / np.sqrt(V)
                if exact_cutoff is not None:
                    hit = np.abs(zz) >= exact_cutoff
                    V = np.where(hit, np.sum(xu * (xu @ nr[c]["P"]), 1) / s2, V)
                    zz = U / np.sqrt(V)
                    flag[b0:b1, c] = hit
            score[b0:b1, c], var[b0:b1, c], z[b0:b1, c] = np.where(valid[b0:b1], U, np.nan), V, zz
    with np.errstate(all="ignore"):
        return dict(score=score, var=var, z=z, pval=erfc_vec(np.abs(z) / np.sqrt(2.0)), beta=score / var, se=1.0 / np.sqrt(var), flag=flag, h2=h2, gamma=gamma,
                    kappa=kappa, nulls=nulls)


def ols_ref(codes, Y, W=None):
    """z (snps, n) of the plain score test y ~ C + x without K: U = x^T M y / s2, V = x^T M x / s2, s2 = y^T M y / (indiv - q - 1)"""
    codes = np.asarray(codes)
    indiv = codes.shape[1]
    Y = np.asarray(Y, np.float64).reshape(indiv, -1)
    _, Qc = design(indiv, W)
    M = np.eye(indiv) - Qc @ Qc.T
    x, valid = imputed(codes)
    MY = M @ Y
    s2 = np.sum(Y * MY, 0) / (indiv - Qc.shape[1])
    with np.errstate(all="ignore"):
        z = (x @ MY) / np.sqrt(np.sum(x * (x @ M), 1)[:, None] * s2[None, :])
    return np.where(valid[:, None], z, np.nan)


def lambda_gc(z):
    z = np.asarray(z, np.float64).reshape(-1)
    return float(np.median(z[np.isfinite(z)] ** 2) / 0.4549)


def structured_case(indiv=401, snps=1200, seed=0, fst=0.05, shift=1.0, h2g=0.4, causal=300):
    """(codes (snps, indiv), y (indiv,), pop (indiv,)): two sub-populations whose allele frequencies differ (Balding-Nichols with F = fst around ancestral
    frequencies U(0.1, 0.9)), crossed with sib-ships of 4 (two parents drawn in the sib-ship's sub-population, every child one allele of each per SNP; a last
    incomplete sib-ship where 4 does not divide indiv).  y = shift pop + g + e: g from `causal` further SNPs of the same pedigree that are NOT among the
    tested ones -- every tested SNP is null --, scaled to variance h2g, e ~ N(0, 1 - h2g).  No missing calls."""
    rng = np.random.default_rng([seed, indiv, snps, 5])
    total = snps + causal
    fam = np.arange(indiv) // 4
    nfam = int(fam[-1]) + 1
    fam_pop = (np.arange(nfam) % 2).astype(np.int64)
    pop = fam_pop[fam]
    p0 = rng.uniform(0.1, 0.9, total)
    a = (1.0 - fst) / fst
    pk = np.stack([rng.beta(p0 * a, (1.0 - p0) * a) for _ in range(2)])                       # (2, total)
    parents = rng.random((nfam, 2, 2, total)) < pk[fam_pop][:, None, None, :]                 # family, parent, haplotype, SNP
    pick = rng.integers(0, 2, (indiv, 2, total))
    geno = np.zeros((indiv, total), np.int64)
    for par in range(2):
        hap = parents[fam, par]                                                                # (indiv, 2, total)
        geno += np.where(pick[:, par] == 0, hap[:, 0], hap[:, 1])
    zc = geno[:, snps:].astype(np.float64)
    g = (zc - zc.mean(0)) @ rng.standard_normal(causal)
    g = g - pop * (g[pop == 1].mean() - g[pop == 0].mean())                                    # the sub-population shift is `shift` alone
    g = g / g.std() * np.sqrt(h2g)
    y = shift * pop + g + np.sqrt(1.0 - h2g) * rng.standard_normal(indiv)
    return np.ascontiguousarray(geno[:, :snps].T), y, pop
