"""Mixed-model association on the genotype operator: y = C gamma + g + e with g ~ N(0, sg2 K), e ~ N(0, se2 I) and K the genomic relationship matrix, never
formed.  Built on existing device entries only: every K v is mxa_gram_matvec_device on a centred compressed object (dgemm_compressed.gram_matvec), every scan
is mxa_assoc_score (assoc.assoc_score); what runs between them per iteration -- the vector updates of the solver, the decodes of a few hundred SNPs, the small
products with the covariates -- are torch operations on fp64 device tensors.

Kinship            K V = sum_b Zc_b Zc_b^T V / sum_b s_b over chromosome blocks, any of which can be left out (LOCO)
solve              block conjugate gradients for (tau K + I) X = B, columns in lockstep with stopping decisions of their own
assoc_mixed_null   h2 by randomized Haseman-Elston regression, the GLS fit of the covariates, r = P y and sigma2
assoc_mixed        the scan: per block the null model, the GRAMMAR-Gamma calibration factor, assoc_score, and optionally exact variances for the top SNPs

V = tau K + I throughout (the phenotypic covariance up to se2), P = V^-1 - V^-1 C (C^T V^-1 C)^-1 C^T V^-1.  The definitions: DESIGN.md 3.6j."""
from collections import namedtuple

import numpy as np

from . import assoc as _assoc
from . import dgemm_compressed as _dg
from . import lib as _lib
from . import read_plink as _rp

MixedNull = namedtuple("MixedNull", "h2 tau gamma r sigma2 VinvC G_chol Qc iters")
AssocMixedResult = namedtuple("AssocMixedResult", "score var zstat pval beta se flag h2 gamma nobs")
EXACT_BATCH = 256            # columns per solve of the exact stage


# ---------------------------------------------------------------------------------------------------------- argument checks (host only, no library call)
def _check_matrix(plink, snps, indiv):
    snps, indiv = int(snps), int(indiv)
    if snps < 1 or indiv < 1:
        raise ValueError(f"snps and indiv need to be positive: {snps}, {indiv}")
    if indiv > _assoc.ASSOC_MAX_INDIV:
        raise ValueError(f"indiv needs to be at most {_assoc.ASSOC_MAX_INDIV}: {indiv}")
    shape = tuple(plink.shape)
    if len(shape) != 2 or shape != (snps, (indiv + 3) // 4):
        raise ValueError(f"Matrix has wrong dimensions: {shape} for snps={snps} indiv={indiv}")
    if not str(plink.dtype).endswith("uint8"):
        raise ValueError(f"plink needs to be uint8: {plink.dtype}")
    return snps, indiv


def _check_bounds(chrom_bounds, snps):
    """the block offsets [0, b1, ..., snps] as a list of ints"""
    if chrom_bounds is None:
        return [0, snps]
    b = [int(v) for v in np.asarray(chrom_bounds).reshape(-1)]
    if len(b) < 2 or b[0] != 0 or b[-1] != snps:
        raise ValueError(f"chrom_bounds need to start at 0 and to end at snps = {snps}: {b}")
    if any(b[i + 1] <= b[i] for i in range(len(b) - 1)):
        raise ValueError(f"chrom_bounds need to be ascending: {b}")
    if any(v % 4 for v in b[:-1]):
        raise ValueError(f"chrom_bounds need to be multiples of 4, except the last: {b}")
    return b


def _check_design(indiv, Y, covariates):
    """(Y as given with two dimensions, n, C = [1 | W] (indiv, q + 1) numpy, Qc numpy): the checks of Y and the covariates that need no device, and the
    orthonormal basis Qc of C by Gram-Schmidt applied twice, in place order.  A device Y is checked for non-finite entries by the caller's first device read."""
    shape = tuple(Y.shape)
    if len(shape) not in (1, 2) or shape[0] != indiv or (len(shape) == 2 and shape[1] < 1):
        raise ValueError(f"Y needs to be ({indiv},) or ({indiv}, n >= 1): {shape}")
    n = 1 if len(shape) == 1 else int(shape[1])
    if _lib.is_torch_tensor(Y):
        if not str(Y.dtype).endswith("float64"):
            raise ValueError(f"Y needs to be float64: {Y.dtype}")
        if not Y.is_cuda and not bool(Y.isfinite().all()):
            raise ValueError("Y needs to be finite")
        Y2 = Y.reshape(indiv, n)
    else:
        Y2 = np.asarray(Y, dtype=np.float64).reshape(indiv, n)
        if not np.all(np.isfinite(Y2)):
            raise ValueError("Y needs to be finite")
    C = np.ones((indiv, 1))
    if covariates is not None:
        W = np.asarray(covariates, dtype=np.float64)
        if W.ndim == 1:
            W = W.reshape(-1, 1)
        if W.ndim != 2 or W.shape[0] != indiv:
            raise ValueError(f"covariates need to be ({indiv}, q) or ({indiv},): {W.shape}")
        if not np.all(np.isfinite(W)):
            raise ValueError("covariates need to be finite")
        C = np.concatenate([C, W], axis=1)
    q = C.shape[1] - 1
    if indiv <= q + 2:
        raise ValueError(f"indiv needs to exceed q + 2: indiv {indiv}, q {q}")
    return Y2, n, C, gram_schmidt_twice(C)


def gram_schmidt_twice(C):
    """Qc (indiv, k): column j is C's column j made orthogonal to the columns before it by Gram-Schmidt applied twice, then scaled to norm 1; float64 on the
    host.  A column whose norm after the two passes is at most indiv 2^-52 times its own is dependent (behind the leading 1: a constant covariate): ValueError."""
    C = np.asarray(C, dtype=np.float64)
    indiv, k = C.shape
    Q = np.zeros((indiv, k))
    for j in range(k):
        v = C[:, j].copy()
        norm0 = np.sqrt(v @ v)
        for _ in range(2):
            for p in range(j):
                v -= (Q[:, p] @ v) * Q[:, p]
        nrm = np.sqrt(v @ v)
        if not nrm > indiv * 2.0 ** -52 * norm0:
            raise ValueError(f"covariate {j - 1} is constant or depends on the covariates before it" if j else "the intercept column is zero")
        Q[:, j] = v / nrm
    return Q


def _check_h2(h2, n):
    """None, or (n,) float64 in [0, 1)"""
    if h2 is None:
        return None
    h = np.asarray(h2, dtype=np.float64).reshape(-1)
    if h.size == 1:
        h = np.repeat(h, n)
    if h.size != n:
        raise ValueError(f"h2 needs to be a scalar or one value per trait: {h.size} values, n = {n}")
    if not np.all((h >= 0) & (h < 1)):
        raise ValueError(f"h2 needs to lie in [0, 1): {h.tolist()}")
    return h


def _check_solver(tol, max_iter):
    tol, max_iter = float(tol), int(max_iter)
    if not 0 < tol < 1:
        raise ValueError(f"tol needs to lie in (0, 1): {tol}")
    if max_iter < 1:
        raise ValueError(f"max_iter needs to be at least 1: {max_iter}")
    return tol, max_iter


def rademacher(indiv, probes, seed):
    """(indiv, probes) float64 of -1 / +1, column-major, drawn on the CPU -- torch.Generator().manual_seed(seed), randint(0, 2, (probes, indiv)) -- so that the
    probes are the same on every machine"""
    import torch
    g = torch.Generator().manual_seed(int(seed))
    return (torch.randint(0, 2, (int(probes), int(indiv)), generator=g, dtype=torch.int64).to(torch.float64) * 2.0 - 1.0).t()


def calibration_picks(size, count, seed, unit):
    """the min(count, size) SNPs of scan unit `unit` (of `size` SNPs) the calibration decodes, ascending offsets into the unit: the head of a CPU randperm
    seeded with seed + 7919 (unit + 1)"""
    import torch
    g = torch.Generator().manual_seed(int(seed) + 7919 * (int(unit) + 1))
    return np.sort(torch.randperm(int(size), generator=g)[:min(int(count), int(size))].numpy())


# ---------------------------------------------------------------------------------------------------------- the kinship operator
class Kinship:
    """K = sum_b Zc_b Zc_b^T / sum_b s_b as an operator on device vectors; K itself is never formed.

    plink: snps rows of ceil(indiv / 4) bytes in PLINK coding, a numpy uint8 array or a torch uint8 tensor (host or device).  chrom_bounds: ascending SNP
    offsets [0, b1, ..., snps] of the chromosome blocks, each a multiple of 4 except the last (None: one block).  freq: the allele frequencies f (snps,), numpy
    or torch (None: read_plink.calc_freq per block).  One centred compressed object is staged per block (init_compressed with plink_transposed=None), with
    s_b = 2 sum f (1 - f) over the block's SNPs.

    Zc is the library's own centred operand: z - 2 f with z the allele count and a MISSING call counted as z = 0 BEFORE centring, so that a missing call
    contributes -2 f (not 0, as mean imputation would give), and f the frequency calc_freq returns: sum z / (2 indiv) with missing as 0 as well.

    The process has to be in the centred default, dgemm_compressed.set_options(not_center=False): the option is global, it is read by every product, and it is
    not reset here.  Under not_center=True apply() multiplies with the uncentred matrix and every result of this module is wrong.

    A context manager; free() releases the objects."""

    def __init__(self, plink, snps, indiv, chrom_bounds=None, freq=None):
        self.snps, self.indiv = _check_matrix(plink, snps, indiv)
        self.bounds = _check_bounds(chrom_bounds, self.snps)
        self.nblocks = len(self.bounds) - 1
        if freq is not None and int(np.prod(freq.shape)) != self.snps:
            raise ValueError(f"freq needs {self.snps} entries: {tuple(freq.shape)}")
        import torch
        self.device = plink.device if _lib.is_torch_tensor(plink) and plink.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.objs, self.s = [], []
        try:
            for b in range(self.nblocks):
                b0, b1 = self.bounds[b], self.bounds[b + 1]
                rows = plink[b0:b1]
                f = _rp.calc_freq(rows, b1 - b0, self.indiv) if freq is None else freq.reshape(-1)[b0:b1]
                self.objs.append(_dg.init_compressed(rows, None, b1 - b0, self.indiv, f, 1))
                fh = f.detach().cpu().numpy() if _lib.is_torch_tensor(f) else np.asarray(f, dtype=np.float64)
                self.s.append(float(2.0 * np.sum(fh * (1.0 - fh))))
        except Exception:
            self.free()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False

    def free(self):
        for obj in self.objs:
            _dg.free_compressed(obj)
        self.objs = []

    def blocks(self, leave_out=None):
        if leave_out is None:
            return list(range(self.nblocks))
        if not 0 <= int(leave_out) < self.nblocks or self.nblocks < 2:
            raise ValueError(f"leave_out needs to name one of at least 2 blocks: {leave_out}, {self.nblocks} blocks")
        return [b for b in range(self.nblocks) if b != int(leave_out)]

    def scale(self, leave_out=None):
        """sum_b s_b over the blocks that take part"""
        total = 0.0
        for b in self.blocks(leave_out):
            total += self.s[b]
        return total

    def apply(self, V, leave_out=None):
        """K V (indiv, n), a column-major fp64 tensor on the object's device, for V (indiv, n) there: the products of the blocks b != leave_out are enqueued
        without a host wait (gram_matvec(..., sync=False)), added in ascending block order and divided by the sum of their s_b."""
        if not self.objs:
            raise RuntimeError("the kinship operator has been freed")
        if not (_lib.is_torch_tensor(V) and V.is_cuda and V.dim() == 2 and V.shape[0] == self.indiv and str(V.dtype).endswith("float64")):
            raise ValueError(f"V needs to be a float64 ({self.indiv}, n) tensor on the device")
        total = None
        for b in self.blocks(leave_out):
            part = _dg.gram_matvec(self.objs[b], V, self.bounds[b + 1] - self.bounds[b], self.indiv, sync=False)
            total = part if total is None else total.add_(part)
        return total.div_(self.scale(leave_out))


# ---------------------------------------------------------------------------------------------------------- the block CG
def _colmajor_zeros(torch, rows, cols, device):
    return torch.zeros((cols, rows), dtype=torch.float64, device=device).t()


def solve(kin, tau, B, leave_out=None, tol=1e-10, max_iter=500):
    """(X, iters, relres): (tau K + I) X = B by conjugate gradients from X = 0, for B (indiv, n), an fp64 tensor on kin's device.  The columns run in lockstep,
    one kin.apply per iteration, each with its own alpha and beta and its own stopping decision |r_c| <= tol |b_c|, taken before the first iteration too (a
    zero column takes none); a finished column is frozen (alpha = 0).  The host reads one number per iteration: the count of running columns.  iters (n,)
    int64 and relres (n,) = |r_c| / |b_c| of the recurrence (0 for a zero column) are device tensors.  A column that is still running after max_iter
    iterations, or that meets p^T A p <= 0, is a RuntimeError that names it."""
    import torch
    tol, max_iter = _check_solver(tol, max_iter)
    tau = float(tau)
    if not tau >= 0:
        raise ValueError(f"tau must not be negative or NaN: {tau}")
    if not (_lib.is_torch_tensor(B) and B.is_cuda and B.dim() == 2 and B.shape[0] == kin.indiv and B.dtype == torch.float64):
        raise ValueError(f"B needs to be a float64 ({kin.indiv}, n) tensor on the device")
    n = B.shape[1]
    X = _colmajor_zeros(torch, kin.indiv, n, B.device)
    R = _colmajor_zeros(torch, kin.indiv, n, B.device).copy_(B)
    P = R.clone()
    rs = (R * R).sum(0)
    bnorm = rs.sqrt()
    thr = tol * bnorm
    active = bnorm > thr
    bad = torch.zeros_like(active)
    iters = torch.zeros(n, dtype=torch.int64, device=B.device)
    zero = torch.zeros_like(rs)
    for it in range(max_iter + 1):
        code = int((active.sum() + (n + 1) * bad.sum()).item())          # the one host read of the iteration
        if code > n:
            col = int(torch.nonzero(bad)[0])
            raise RuntimeError(f"mixed.solve: p^T A p <= 0 in column {col} at iteration {it}: the operator is not positive definite")
        if code == 0:
            break
        if it == max_iter:
            col = int(torch.nonzero(active)[0])
            raise RuntimeError(f"mixed.solve: column {col} has not converged after {max_iter} iterations: |r| / |b| = {float(rs[col].sqrt() / bnorm[col]):.3e}, "
                               f"tol {tol:.3e}")
        AP = kin.apply(P, leave_out).mul_(tau).add_(P)
        pAp = (P * AP).sum(0)
        bad = active & ~(pAp > 0)
        alpha = torch.where(active & ~bad, rs / pAp, zero)
        X.add_(P * alpha)
        R.sub_(AP * alpha)
        rs_new = (R * R).sum(0)
        beta = torch.where(active, rs_new / rs, zero)
        P = R + P * beta
        iters += active
        rs = torch.where(active, rs_new, rs)
        active = active & (rs.sqrt() > thr)
    relres = torch.where(bnorm > 0, rs.sqrt() / bnorm, zero)
    return X, iters, relres


# ---------------------------------------------------------------------------------------------------------- the null model
def _to_device(torch, a, device):
    """a column-major fp64 device copy of a 2-D host / device matrix"""
    t = a if _lib.is_torch_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    out = torch.empty((t.shape[1], t.shape[0]), dtype=torch.float64, device=device).t()
    return out.copy_(t)


def _project(Qc, V):
    """M V = V - Qc (Qc^T V)"""
    return V - Qc @ (Qc.t() @ V)


def haseman_elston(kin, Y, Qc, probes=32, seed=1, leave_out=None):
    """h2 (n,) numpy by randomized Haseman-Elston regression for Y (indiv, n) and the orthonormal Qc (indiv, q + 1), device tensors: with y~ = M y,
    K~ = M K M and Rademacher probes z_b (rademacher(indiv, probes, seed)), t1 = mean_b z_b^T K~ z_b and t2 = mean_b |K~ z_b|^2, the solution of
    [[t2, t1], [t1, N - q - 1]] [sg2, se2]^T = [y~^T K~ y~, y~^T y~]^T gives h2 = sg2 / (sg2 + se2), clipped to [0, 0.999].  One kin.apply of n + probes columns."""
    import torch
    indiv, n = Y.shape
    k = Qc.shape[1]
    Z = rademacher(indiv, probes, seed).to(Y.device)
    MV = _project(Qc, torch.cat([Y, Z], dim=1))
    KV = kin.apply(MV, leave_out)
    MKV = _project(Qc, KV)
    quad = (MV * KV).sum(0).cpu().numpy()                 # v^T M K M v
    sq = (MKV * MKV).sum(0).cpu().numpy()                 # |M K M v|^2
    yy = (MV[:, :n] * MV[:, :n]).sum(0).cpu().numpy()
    t1, t2 = float(np.mean(quad[n:])), float(np.mean(sq[n:]))
    dof = float(indiv - k)
    det = t2 * dof - t1 * t1
    sg2 = (dof * quad[:n] - t1 * yy) / det
    se2 = (t2 * yy - t1 * quad[:n]) / det
    h2 = sg2 / (sg2 + se2)
    if not np.all(np.isfinite(h2)):
        raise RuntimeError(f"the Haseman-Elston system is degenerate: t1 {t1}, t2 {t2}, sg2 {sg2.tolist()}, se2 {se2.tolist()}")
    return np.clip(h2, 0.0, 0.999)


def _gls(kin, Yd, Cd, tau, leave_out, tol, max_iter):
    """the GLS fit of every trait: one solve of [y's | C] per distinct tau"""
    import torch
    indiv, n = Yd.shape
    k = Cd.shape[1]
    gamma, sigma2, iters = np.zeros((k, n)), np.zeros(n), np.zeros(n, dtype=np.int64)
    chol = np.zeros((n, k, k))
    r = _colmajor_zeros(torch, indiv, n, Yd.device)
    VinvC = [None] * n
    for t in np.unique(tau):
        cols = [c for c in range(n) if tau[c] == t]
        X, its, _ = solve(kin, t, torch.cat([Yd[:, cols], Cd], dim=1), leave_out, tol, max_iter)
        VY, VC = X[:, :len(cols)], X[:, len(cols):]
        G = (Cd.t() @ VC).cpu().numpy()
        G = 0.5 * (G + G.T)
        L = np.linalg.cholesky(G)
        g = np.linalg.solve(L.T, np.linalg.solve(L, (Cd.t() @ VY).cpu().numpy()))           # (k, len(cols))
        rt = VY - VC @ torch.from_numpy(g).to(Yd.device)
        s2 = ((Yd[:, cols] * rt).sum(0) / float(indiv - k)).cpu().numpy()
        its = its.cpu().numpy()
        for j, c in enumerate(cols):
            gamma[:, c], sigma2[c], iters[c], chol[c], VinvC[c] = g[:, j], s2[j], its[j], L, VC
            r[:, c] = rt[:, j]
    return gamma, r, sigma2, VinvC, chol, iters


def assoc_mixed_null(kin, Y, covariates=None, h2=None, probes=32, seed=1, leave_out=None, tol=1e-10, max_iter=500):
    """The null model y_c = C gamma_c + g + e, C = [1 | covariates], of every column of Y ((indiv, n) or (indiv,), float64, numpy or torch, host or device) on
    the kinship operator kin, without the block leave_out when one is named.  h2: None (haseman_elston with `probes` probes and `seed`, per trait), or a
    scalar or one value per trait in [0, 1), used as it is.  tau = h2 / (1 - h2), V = tau K + I.  Per distinct tau one solve() of [y | C] gives G = C^T V^-1 C
    (factored on the host), gamma = G^-1 C^T V^-1 y, r = V^-1 y - V^-1 C gamma = P y and sigma2 = y^T r / (indiv - q - 1).
    Returns MixedNull: h2, tau, sigma2 (n,), gamma (q + 1, n), G_chol (n, q + 1, q + 1) lower factors and iters (n,), the iterations of y's column, as numpy;
    r (indiv, n) and Qc (indiv, q + 1), the orthonormal basis of C (gram_schmidt_twice), as device tensors; VinvC: per trait the device tensor V^-1 C
    (indiv, q + 1), shared by the traits of one tau.  Argument errors are ValueErrors raised before the first library call."""
    import torch
    indiv = int(kin.indiv)
    Y2, n, C, Qc = _check_design(indiv, Y, covariates)
    hv = _check_h2(h2, n)
    if int(probes) < 1:
        raise ValueError(f"probes needs to be at least 1: {probes}")
    tol, max_iter = _check_solver(tol, max_iter)
    if leave_out is not None:
        kin.blocks(leave_out)
    Yd = _to_device(torch, Y2, kin.device)
    if _lib.is_torch_tensor(Y) and Y.is_cuda and not bool(Yd.isfinite().all()):
        raise ValueError("Y needs to be finite")
    Cd, Qd = _to_device(torch, C, kin.device), _to_device(torch, Qc, kin.device)
    if hv is None:
        hv = haseman_elston(kin, Yd, Qd, int(probes), seed, leave_out)
    return _null(kin, Yd, Cd, Qd, hv, leave_out, tol, max_iter)


def _null(kin, Yd, Cd, Qd, h2, leave_out, tol, max_iter):
    """MixedNull from checked device operands and h2 (n,)"""
    tau = h2 / (1.0 - h2)
    gamma, r, sigma2, VinvC, chol, iters = _gls(kin, Yd, Cd, tau, leave_out, tol, max_iter)
    return MixedNull(h2, tau, gamma, r, sigma2, VinvC, chol, Qd, iters)


# ---------------------------------------------------------------------------------------------------------- the scan
def decode_imputed(rows, indiv):
    """(x (indiv, m) fp64 column-major, valid (m,) bool) of m packed SNP rows (a uint8 device tensor (m, ceil(indiv / 4))): the allele counts with missing
    calls replaced by the SNP's mean over its called individuals, as mxa_assoc_score reads them; a SNP without a called individual or without variance among
    the called ones is not valid and decodes to a zero column."""
    import torch
    r = rows.to(torch.int32)
    codes = torch.stack([(r >> s) & 3 for s in (0, 2, 4, 6)], dim=2).reshape(rows.shape[0], -1)[:, :indiv]
    called = codes != 1
    z = torch.where(codes >= 2, codes - 1, torch.zeros_like(codes)).to(torch.float64)
    N = called.sum(1).to(torch.float64)
    Sz, Szz = z.sum(1), (z * z).sum(1)
    valid = (N > 0) & (N * Szz - Sz * Sz > 0)
    mu = torch.where(valid, Sz / N, torch.zeros_like(Sz))
    x = torch.where(called, z, mu[:, None]) * valid[:, None]
    return x.t(), valid


def _packed_rows(torch, plink, idx, device):
    """the packed rows idx of the PLINK matrix as a device tensor"""
    if _lib.is_torch_tensor(plink):
        return plink.index_select(0, torch.as_tensor(idx, dtype=torch.int64, device=plink.device)).to(device)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(plink)[idx])).to(device)


def _quad_P(kin, null, c, X, leave_out, tol, max_iter):
    """x_l^T P x_l (m,) of the columns of X under trait c's null model: one block solve"""
    import torch
    VX, _, _ = solve(kin, null.tau[c], X, leave_out, tol, max_iter)
    L = null.G_chol[c]
    T = (null.VinvC[c].t() @ X).cpu().numpy()                                  # (q + 1, m)
    S = torch.from_numpy(np.linalg.solve(L.T, np.linalg.solve(L, T))).to(X.device)
    return (X * (VX - null.VinvC[c] @ S)).sum(0)


def assoc_mixed(plink, snps, indiv, Y, covariates=None, chrom_bounds=None, loco=True, h2=None, calib_snps=200, exact_cutoff=None, seed=1, probes=32,
                tol=1e-10, max_iter=500):
    """The mixed-model score test of every SNP for the columns of Y, calibrated as GRAMMAR-Gamma does.

    plink: snps rows of ceil(indiv / 4) bytes in PLINK coding, numpy uint8 or a torch uint8 tensor (host or device).  Y: (indiv, n) or (indiv,) float64, numpy
    or torch (host or device); covariates: (indiv, q) numpy or None.  chrom_bounds: as for Kinship.  h2: None -- estimated ONCE on the full K
    (haseman_elston) and shared by the blocks --, or given (assoc_mixed_null).

    With loco=True and at least 2 blocks, block c is scanned under the null model fitted without it (leave_out=c); otherwise (a single block included: loco
    then falls back to False) the whole matrix is scanned under one null model.  Per scan unit u and trait:
      null         assoc_mixed_null: r = P y, sigma2, V^-1 C, G
      calibration  min(calib_snps, size) SNPs of the unit (calibration_picks), decoded with missing calls as the SNP's mean (SNPs without a called individual
                   or without variance are skipped), P x_l from one block solve, gamma_u = sum_l x_l^T P x_l / sum_l x_l^T M x_l
      scan         assoc_score on the unit's rows with R = r / sigma2, Wt = gamma_u / sigma2 and H = sqrt(gamma_u / sigma2) Qc: U = x^T P y / sigma2,
                   V = gamma_u x^T M x / sigma2, z = U / sqrt(V)
      exact stage  (exact_cutoff given) for every (SNP, trait) with |z| >= exact_cutoff the SNP is decoded and solved, in batches of at most 256 columns, and
                   V = x^T P x / sigma2 replaces the calibrated value, z with it; flag is 1 there and 0 elsewhere
    Returns AssocMixedResult(score, var, zstat, pval = erfc(|z| / sqrt 2), beta = U / V, se = 1 / sqrt(V), flag (int32), h2 (n,), gamma (units, n), nobs
    (snps,) int32): the SNP arrays are (snps, n), device tensors when plink is a device tensor and numpy arrays otherwise; gamma has one row per scan unit, so
    (1, n) says that no block was left out.  Non-finite statistics mark SNPs without information, as for assoc_score.  The process has to be in the centred
    default (Kinship).  Argument errors are ValueErrors raised before the first library call."""
    import torch
    snps, indiv = _check_matrix(plink, snps, indiv)
    bounds = _check_bounds(chrom_bounds, snps)
    Y2, n, C, Qc = _check_design(indiv, Y, covariates)
    hv = _check_h2(h2, n)
    if int(probes) < 1:
        raise ValueError(f"probes needs to be at least 1: {probes}")
    if int(calib_snps) < 1:
        raise ValueError(f"calib_snps needs to be at least 1: {calib_snps}")
    if exact_cutoff is not None and not float(exact_cutoff) >= 0:
        raise ValueError(f"exact_cutoff must not be negative or NaN: {exact_cutoff}")
    tol, max_iter = _check_solver(tol, max_iter)
    loco = bool(loco) and len(bounds) > 2
    units = [(c, bounds[c], bounds[c + 1]) for c in range(len(bounds) - 1)] if loco else [(None, 0, snps)]
    on_device = _lib.is_torch_tensor(plink) and plink.is_cuda
    with Kinship(plink, snps, indiv, bounds) as kin:
        dev = kin.device
        Yd = _to_device(torch, Y2, dev)
        if _lib.is_torch_tensor(Y) and Y.is_cuda and not bool(Yd.isfinite().all()):
            raise ValueError("Y needs to be finite")
        Cd, Qd = _to_device(torch, C, dev), _to_device(torch, Qc, dev)
        if hv is None:
            hv = haseman_elston(kin, Yd, Qd, int(probes), seed, None)
        parts = {key: [] for key in ("score", "var", "z", "flag", "nobs")}
        gammas = np.zeros((len(units), n))
        for u, (leave, b0, b1) in enumerate(units):
            null = _null(kin, Yd, Cd, Qd, hv, leave, tol, max_iter)
            rows_u = plink[b0:b1]
            X, _ = decode_imputed(_packed_rows(torch, rows_u, calibration_picks(b1 - b0, calib_snps, seed, u), dev), indiv)
            QX = Qd.t() @ X
            den = float(((X * X).sum() - (QX * QX).sum()).item())
            if not den > 0:
                raise RuntimeError(f"no calibration SNP of scan unit {u} carries information")
            for t in np.unique(null.tau):
                cols = [c for c in range(n) if null.tau[c] == t]
                gammas[u, cols] = float(_quad_P(kin, null, cols[0], X, leave, tol, max_iter).sum().item()) / den
            del X, QX
            scale = torch.from_numpy(gammas[u] / null.sigma2).to(dev)                       # gamma_u / sigma2 per trait
            R = null.r / torch.from_numpy(null.sigma2).to(dev)
            Wt = _colmajor_zeros(torch, indiv, n, dev).add_(scale)
            H = torch.cat([Qd * scale[c].sqrt() for c in range(n)], dim=1)
            res = _assoc.assoc_score(rows_u, b1 - b0, indiv, R, Wt, H)
            score, var, z = res.score.contiguous(), res.var.contiguous(), res.z.contiguous()
            flag = torch.zeros((b1 - b0, n), dtype=torch.int32, device=dev)
            if exact_cutoff is not None:
                hits = torch.nonzero(z.abs() >= float(exact_cutoff)).cpu().numpy()          # (count, 2): SNP of the unit, trait
                for c in range(n):
                    idx = hits[hits[:, 1] == c, 0]
                    for at in range(0, idx.size, EXACT_BATCH):
                        sel = idx[at:at + EXACT_BATCH]
                        Xe, _ = decode_imputed(_packed_rows(torch, rows_u, sel, dev), indiv)
                        v = _quad_P(kin, null, c, Xe, leave, tol, max_iter) / float(null.sigma2[c])
                        seld = torch.as_tensor(sel, dtype=torch.int64, device=dev)
                        var[seld, c] = v
                        z[seld, c] = score[seld, c] / v.sqrt()
                        flag[seld, c] = 1
            for key, a in (("score", score), ("var", var), ("z", z), ("flag", flag)):
                parts[key].append(a)
            parts["nobs"].append(res.nobs)
        score, var, z, flag = (torch.cat(parts[key], dim=0) for key in ("score", "var", "z", "flag"))
        pval = torch.special.erfc(z.abs() / np.sqrt(2.0))
        beta, se = score / var, 1.0 / var.sqrt()
        out = [score, var, z, pval, beta, se, flag]
        if not on_device:
            out = [a.cpu().numpy() for a in out]
    return AssocMixedResult(*out, np.asarray(hv, dtype=np.float64), gammas, np.concatenate(parts["nobs"]))
