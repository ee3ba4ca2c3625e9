"""Association scan (C entries mxa_assoc_basis, mxa_assoc_linear): per-SNP linear regression y ~ 1 + covariates + x_s on packed genotypes, missing calls
imputed by the SNP's mean; and, for binary traits, the score test of a logistic null model fitted once per trait (mxa_assoc_logistic_null, mxa_assoc_score),
with saddlepoint p-values for unbalanced case-control data (mxa_assoc_score_spa) and with effect sizes by Firth-penalised fits (mxa_assoc_score_firth);
and the burden and SKAT tests of SNP sets under the same null models (mxa_assoc_set, mxa_assoc_skat_pvalue).
The definitions, the operation orders and what is exact: include/miraculix_amd.h."""
import ctypes
from collections import namedtuple

import numpy as np

from . import lib as _lib

ASSOC_MAX_INDIV = 47453132          # 4 indiv^2 < 2^53
AssocResult = namedtuple("AssocResult", "beta se t nobs dof")


def _check(rc, entry):
    if rc != 0:
        raise RuntimeError(f"{entry} failed: " + _lib.last_error()[1])


def assoc_basis(covariates):
    """Q (indiv, q), float64 in Fortran order: the centred columns of `covariates` (indiv, q) or (indiv,), orthonormalised in place order by Gram-Schmidt applied
    twice on the host.  The columns of Q are orthonormal and sum to zero: what assoc_linear(Q=...) expects.  A constant or dependent column is an error."""
    W = np.asarray(covariates, dtype=np.float64)
    if W.ndim == 1:
        W = W.reshape(-1, 1)
    if W.ndim != 2 or W.shape[0] < 1:
        raise ValueError(f"covariates need to be (indiv, q) or (indiv,): {W.shape}")
    indiv, q = W.shape
    Q = np.zeros((indiv, q), dtype=np.float64, order="F")
    if q == 0:
        return Q
    if not np.all(np.isfinite(W)):
        raise ValueError("covariates need to be finite")
    Wf = np.asfortranarray(W)
    L = _lib.check_library_handle()
    _check(L.mxa_assoc_basis(int(indiv), _lib.ptr(Wf), int(indiv), int(q), _lib.ptr(Q), int(indiv)), "mxa_assoc_basis")
    return Q


def _columns(x, rows, what):
    """(column-major operand, number of columns): a (cols, rows) C-contiguous array / tensor whose memory is the (rows, cols) column-major matrix"""
    shape = tuple(x.shape)
    if len(shape) not in (1, 2) or shape[0] != rows or (len(shape) == 2 and shape[1] < 1):
        raise ValueError(f"{what} needs to be ({rows},) or ({rows}, n >= 1): {shape}")
    cols = 1 if len(shape) == 1 else int(shape[1])
    if _lib.is_torch_tensor(x):
        import torch
        if x.dtype != torch.float64:
            raise ValueError(f"{what} needs to be float64")
        return x.reshape(rows, cols).t().contiguous(), cols
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(rows, cols).T), cols


def assoc_linear(plink, snps, indiv, Y, covariates=None, Q=None, out=None):
    """beta, se, t (each (snps, n), or (snps,) for a one-dimensional Y), nobs (snps,) int32 and dof of the regressions y_c ~ 1 + covariates + x_s for every SNP s.
    plink: snps rows of ceil(indiv / 4) bytes in PLINK coding, numpy uint8 or a torch uint8 tensor (host / device).  Y: (indiv, n) or (indiv,) float64, numpy or
    torch.  covariates: (indiv, q) raw covariates (numpy; assoc_basis is applied), or Q: an orthonormal zero-sum basis as assoc_basis returns it (numpy or
    torch); at most one of the two.  The results are numpy arrays, or torch tensors on Y's device when Y is a device tensor.  out: a dict with any of the keys
    "beta", "se", "t" -> (snps, n) float64 results to fill (Fortran-ordered numpy, or torch tensors whose transpose is contiguous; all of one kind); statistics
    without a key are then not computed and returned as None.  Non-finite results mark SNPs without information (no called individual, constant, or in the span
    of the covariates): filter them."""
    snps, indiv = int(snps), int(indiv)
    if snps < 1 or indiv < 1:
        raise ValueError(f"snps and indiv need to be positive: {snps}, {indiv}")
    if indiv > ASSOC_MAX_INDIV:
        raise ValueError(f"indiv needs to be at most {ASSOC_MAX_INDIV}: {indiv}")
    if int(np.prod(plink.shape)) != snps * ((indiv + 3) // 4):
        raise ValueError(f"Matrix has wrong dimensions: {tuple(plink.shape)}")
    if covariates is not None and Q is not None:
        raise ValueError("at most one of covariates and Q is needed")
    yc, n = _columns(Y, indiv, "Y")
    if covariates is not None:
        W = np.asarray(covariates)
        if W.ndim not in (1, 2) or W.shape[0] != indiv:
            raise ValueError(f"covariates need to be ({indiv}, q): {W.shape}")
        if indiv - (1 if W.ndim == 1 else W.shape[1]) - 2 < 1:
            raise ValueError(f"indiv - k - 2 degrees of freedom need to be at least 1: indiv {indiv}, covariates {W.shape}")
        Q = assoc_basis(covariates)
    k = 0
    qc = None
    if Q is not None and not (len(tuple(Q.shape)) == 2 and Q.shape[1] == 0):
        qc, k = _columns(Q, indiv, "Q")
    if indiv - k - 2 < 1:
        raise ValueError(f"indiv - k - 2 degrees of freedom need to be at least 1: indiv {indiv}, k {k}")
    one_dim = len(tuple(Y.shape)) == 1
    on_device = _lib.is_torch_tensor(Y) and Y.is_cuda
    res = {}
    if out is not None:
        if not out or any(key not in ("beta", "se", "t") for key in out):
            raise ValueError("out needs to hold at least one of the keys 'beta', 'se', 't'")
        for key, o in out.items():
            ot = o.t() if _lib.is_torch_tensor(o) else o.T
            ok = tuple(o.shape) == (snps, n) and str(o.dtype).endswith("float64") and (ot.is_contiguous() if _lib.is_torch_tensor(o) else ot.flags.c_contiguous)
            if not ok:
                raise ValueError(f"out[{key!r}] needs to be a float64 ({snps}, {n}) result with contiguous columns")
            res[key] = ot
    else:
        for key in ("beta", "se", "t"):
            if on_device:
                import torch
                res[key] = torch.zeros((n, snps), dtype=torch.float64, device=Y.device)
            else:
                res[key] = np.zeros((n, snps), dtype=np.float64)
    nobs = np.zeros(snps, dtype=np.int32)
    dof = ctypes.c_int(0)
    L = _lib.check_library_handle()
    _check(L.mxa_assoc_linear(_lib.ptr(plink), snps, indiv, _lib.ptr(yc), indiv, n, _lib.ptr(qc), indiv, k, _lib.ptr(res.get("beta")), _lib.ptr(res.get("se")),
                              _lib.ptr(res.get("t")), snps, _lib.ptr(nobs), ctypes.byref(dof)), "mxa_assoc_linear")

    def shaped(key):
        if key not in res:
            return None
        if out is not None:
            return out[key]
        r = res[key].t() if _lib.is_torch_tensor(res[key]) else res[key].T
        return r.reshape(snps) if one_dim else r
    return AssocResult(shaped("beta"), shaped("se"), shaped("t"), nobs, int(dof.value))


# ---- binary traits: the score test (C entries mxa_assoc_logistic_null, mxa_assoc_score)
LogisticNull = namedtuple("LogisticNull", "gamma r w H iters")
AssocScoreResult = namedtuple("AssocScoreResult", "score var z nobs")


def assoc_logistic_null(y, covariates=None, tol=1e-10, max_iter=50):
    """The null model of the score test, on the host: logit P(y = 1) = [1 | covariates] gamma by Newton / IRLS.  y: (indiv,) of exactly 0 and 1; covariates:
    (indiv, q) or (indiv,) or None.  Returns (gamma (q + 1,), r = y - p (indiv,), w = p (1 - p) (indiv,), H (indiv, q + 1) Fortran-ordered, iters): r, w and H
    are what assoc_score takes for this trait.  Separation, a constant or dependent covariate and a y that is not 0 / 1 are errors."""
    yv = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
    if yv.ndim != 1 or yv.shape[0] < 1:
        raise ValueError(f"y needs to be (indiv,): {yv.shape}")
    indiv = yv.shape[0]
    Wf, q = None, 0
    if covariates is not None:
        W = np.asarray(covariates, dtype=np.float64)
        if W.ndim == 1:
            W = W.reshape(-1, 1)
        if W.ndim != 2 or W.shape[0] != indiv:
            raise ValueError(f"covariates need to be ({indiv}, q) or ({indiv},): {W.shape}")
        q = int(W.shape[1])
        Wf = np.asfortranarray(W) if q else None
    if indiv <= q + 1:
        raise ValueError(f"indiv needs to exceed q + 1: indiv {indiv}, q {q}")
    gamma, r, w = np.zeros(q + 1), np.zeros(indiv), np.zeros(indiv)
    H = np.zeros((indiv, q + 1), dtype=np.float64, order="F")
    iters = ctypes.c_int(0)
    L = _lib.check_library_handle()
    _check(L.mxa_assoc_logistic_null(indiv, _lib.ptr(yv), _lib.ptr(Wf), indiv, q, float(tol), int(max_iter), _lib.ptr(gamma), _lib.ptr(r), _lib.ptr(w), _lib.ptr(H),
                                     indiv, ctypes.byref(iters)), "mxa_assoc_logistic_null")
    return LogisticNull(gamma, r, w, H, int(iters.value))


def _score_operands(plink, snps, indiv, R, Wt, H):
    """the checks and the column-major operands of assoc_score and assoc_score_spa: (R, Wt, H or None, n, kh)"""
    if snps < 1 or indiv < 1:
        raise ValueError(f"snps and indiv need to be positive: {snps}, {indiv}")
    if indiv > ASSOC_MAX_INDIV:
        raise ValueError(f"indiv needs to be at most {ASSOC_MAX_INDIV}: {indiv}")
    if int(np.prod(plink.shape)) != snps * ((indiv + 3) // 4):
        raise ValueError(f"Matrix has wrong dimensions: {tuple(plink.shape)}")
    rc, n = _columns(R, indiv, "R")
    wc, nw = _columns(Wt, indiv, "Wt")
    if nw != n:
        raise ValueError(f"Wt needs as many columns as R: {nw}, {n}")
    kh, hc = 0, None
    if H is not None and not (len(tuple(H.shape)) == 2 and H.shape[1] == 0):
        hc, nh = _columns(H, indiv, "H")
        if nh % n:
            raise ValueError(f"H needs n kh columns: {nh} columns, n = {n}")
        kh = nh // n
    if n * (kh + 2) > 65535:
        raise ValueError(f"n (kh + 2) needs to be at most 65535: n {n}, kh {kh}")
    return rc, wc, hc, n, kh


def _score_results(keys, required, out, snps, n, like):
    """the (n, snps) C-contiguous result buffers by key: those of `out` (transposed views), else fresh ones of every key, torch tensors on `like`'s device when
    it is a device tensor.  `required` keys must be in a given out."""
    res = {}
    if out is not None:
        names = ", ".join(repr(k) for k in keys)
        if not out or any(key not in keys for key in out) or any(key not in out for key in required):
            raise ValueError(f"out needs to hold at least one of the keys {names}" + (f" and every one of {required}" if required else ""))
        for key, o in out.items():
            ot = o.t() if _lib.is_torch_tensor(o) else o.T
            ok = tuple(o.shape) == (snps, n) and str(o.dtype).endswith("float64") and (ot.is_contiguous() if _lib.is_torch_tensor(o) else ot.flags.c_contiguous)
            if not ok:
                raise ValueError(f"out[{key!r}] needs to be a float64 ({snps}, {n}) result with contiguous columns")
            res[key] = ot
        return res
    on_device = _lib.is_torch_tensor(like) and like.is_cuda
    for key in keys:
        if on_device:
            import torch
            res[key] = torch.zeros((n, snps), dtype=torch.float64, device=like.device)
        else:
            res[key] = np.zeros((n, snps), dtype=np.float64)
    return res


def _shaped(res, out, key, snps, one_dim):
    if key not in res:
        return None
    if out is not None:
        return out[key]
    r = res[key].t() if _lib.is_torch_tensor(res[key]) else res[key].T
    return r.reshape(snps) if one_dim else r


def assoc_score(plink, snps, indiv, R, Wt, H=None, out=None):
    """score U, var V, z = U / sqrt(V) (each (snps, n), or (snps,) for a one-dimensional R) and nobs (snps,) int32 of the score test of every SNP against the
    null models of n traits.  plink: as for assoc_linear.  R, Wt: (indiv, n) or (indiv,) float64 null residuals and working weights; H: (indiv, n kh) projection
    columns, trait c owning the columns c kh .. c kh + kh - 1 (None: kh = 0); numpy or torch, host or device, each independently.  The results are numpy
    arrays, or torch tensors on R's device when R is a device tensor.  out: a dict with any of the keys "score", "var", "z", as for assoc_linear."""
    snps, indiv = int(snps), int(indiv)
    rc, wc, hc, n, kh = _score_operands(plink, snps, indiv, R, Wt, H)
    one_dim = len(tuple(R.shape)) == 1
    res = _score_results(("score", "var", "z"), (), out, snps, n, R)
    nobs = np.zeros(snps, dtype=np.int32)
    L = _lib.check_library_handle()
    _check(L.mxa_assoc_score(_lib.ptr(plink), snps, indiv, _lib.ptr(rc), indiv, _lib.ptr(wc), indiv, _lib.ptr(hc), indiv, n, kh, _lib.ptr(res.get("score")),
                             _lib.ptr(res.get("var")), _lib.ptr(res.get("z")), snps, _lib.ptr(nobs)), "mxa_assoc_score")
    return AssocScoreResult(*(_shaped(res, out, key, snps, one_dim) for key in ("score", "var", "z")), nobs)


AssocSpaResult = namedtuple("AssocSpaResult", "score var z pval flag nobs")


def assoc_score_spa(plink, snps, indiv, P, R, Wt, H=None, z_cutoff=2.0, tol=2.0 ** -30, max_iter=50, out=None):
    """assoc_score with saddlepoint p-values (C entry mxa_assoc_score_spa): score, var, z and nobs exactly as assoc_score returns them, pval (snps, n) and flag
    (snps, n) int32 -- 0: |z| < z_cutoff, the normal p-value erfc(|z| / sqrt 2); 1: the saddlepoint p-value; 2: the saddlepoint solve did not apply (the
    statistic lies on the edge of its support, or no convergence), the normal p-value; 3: z is not finite, NaN.  P: (indiv, n) or (indiv,) float64, the null
    models' fitted probabilities in (0, 1) (y - r of assoc_logistic_null), numpy or torch like R, Wt and H.  The correction runs on the device for the (SNP,
    trait) pairs with |z| >= z_cutoff only; z_cutoff = inf corrects nothing.  out: a dict with the key "pval" and at least one of "score", "var", "z"."""
    snps, indiv = int(snps), int(indiv)
    rc, wc, hc, n, kh = _score_operands(plink, snps, indiv, R, Wt, H)
    pc, np_ = _columns(P, indiv, "P")
    if np_ != n:
        raise ValueError(f"P needs as many columns as R: {np_}, {n}")
    z_cutoff, tol, max_iter = float(z_cutoff), float(tol), int(max_iter)
    if not z_cutoff >= 0:
        raise ValueError(f"z_cutoff must not be negative or NaN: {z_cutoff}")
    if not 0 < tol < 1:
        raise ValueError(f"tol needs to lie in (0, 1): {tol}")
    if max_iter < 1:
        raise ValueError(f"max_iter needs to be at least 1: {max_iter}")
    one_dim = len(tuple(R.shape)) == 1
    res = _score_results(("score", "var", "z", "pval"), ("pval",), out, snps, n, R)
    if len(res) < 2:
        raise ValueError("out needs to hold one of the keys 'score', 'var', 'z' beside 'pval'")
    if _lib.is_torch_tensor(res["pval"]) and res["pval"].is_cuda:
        import torch
        flag = torch.zeros((n, snps), dtype=torch.int32, device=res["pval"].device)
    else:
        flag = np.zeros((n, snps), dtype=np.int32)
    nobs = np.zeros(snps, dtype=np.int32)
    L = _lib.check_library_handle()
    _check(L.mxa_assoc_score_spa(_lib.ptr(plink), snps, indiv, _lib.ptr(pc), indiv, _lib.ptr(rc), indiv, _lib.ptr(wc), indiv, _lib.ptr(hc), indiv, n, kh, z_cutoff, tol,
                                 max_iter, _lib.ptr(res.get("score")), _lib.ptr(res.get("var")), _lib.ptr(res.get("z")), _lib.ptr(res["pval"]), snps, _lib.ptr(flag),
                                 _lib.ptr(nobs)), "mxa_assoc_score_spa")
    fl = flag.t() if _lib.is_torch_tensor(flag) else flag.T
    return AssocSpaResult(*(_shaped(res, out, key, snps, one_dim) for key in ("score", "var", "z", "pval")), fl.reshape(snps) if one_dim else fl, nobs)


AssocFirthResult = namedtuple("AssocFirthResult", "score var z beta se chisq pval flag nobs")


def assoc_score_firth(plink, snps, indiv, P, R, Wt, H=None, z_cutoff=2.0, penalty=1, tol=2.0 ** -30, max_iter=50, out=None):
    """assoc_score with effect sizes (C entry mxa_assoc_score_firth): score, var, z and nobs exactly as assoc_score returns them; beta (the SNP's log odds
    ratio), se, chisq (the likelihood-ratio statistic), pval (each (snps, n)) and flag (snps, n) int32 -- 0: |z| < z_cutoff, the one-step values U / V,
    1 / sqrt(V), z^2 and the normal p-value; 1: the fit of logit pi = logit p + beta g by Newton on the device, penalty=1: with Firth's penalty (finite where
    carriers and cases separate), penalty=0: maximum likelihood; 2: no fit (penalty=0: the statistic lies on the edge of its support; no convergence), the
    one-step values; 3: z is not finite, NaN.  P, R, Wt, H: as for assoc_score_spa.  z_cutoff = inf fits nothing.  out: a dict with the key "beta", at least
    one of "score", "var", "z" and any of "se", "chisq", "pval"."""
    snps, indiv = int(snps), int(indiv)
    rc, wc, hc, n, kh = _score_operands(plink, snps, indiv, R, Wt, H)
    pc, np_ = _columns(P, indiv, "P")
    if np_ != n:
        raise ValueError(f"P needs as many columns as R: {np_}, {n}")
    z_cutoff, tol, max_iter = float(z_cutoff), float(tol), int(max_iter)
    if not z_cutoff >= 0:
        raise ValueError(f"z_cutoff must not be negative or NaN: {z_cutoff}")
    if penalty not in (0, 1):
        raise ValueError(f"penalty needs to be 0 or 1: {penalty}")
    if not 0 < tol < 1:
        raise ValueError(f"tol needs to lie in (0, 1): {tol}")
    if max_iter < 1:
        raise ValueError(f"max_iter needs to be at least 1: {max_iter}")
    one_dim = len(tuple(R.shape)) == 1
    keys = ("score", "var", "z", "beta", "se", "chisq", "pval")
    res = _score_results(keys, ("beta",), out, snps, n, R)
    if not any(key in res for key in ("score", "var", "z")):
        raise ValueError("out needs to hold one of the keys 'score', 'var', 'z' beside 'beta'")
    if _lib.is_torch_tensor(res["beta"]) and res["beta"].is_cuda:
        import torch
        flag = torch.zeros((n, snps), dtype=torch.int32, device=res["beta"].device)
    else:
        flag = np.zeros((n, snps), dtype=np.int32)
    nobs = np.zeros(snps, dtype=np.int32)
    L = _lib.check_library_handle()
    _check(L.mxa_assoc_score_firth(_lib.ptr(plink), snps, indiv, _lib.ptr(pc), indiv, _lib.ptr(rc), indiv, _lib.ptr(wc), indiv, _lib.ptr(hc), indiv, n, kh, z_cutoff,
                                   int(penalty), tol, max_iter, *(_lib.ptr(res.get(key)) for key in keys), snps, _lib.ptr(flag), _lib.ptr(nobs)),
           "mxa_assoc_score_firth")
    fl = flag.t() if _lib.is_torch_tensor(flag) else flag.T
    return AssocFirthResult(*(_shaped(res, out, key, snps, one_dim) for key in keys), fl.reshape(snps) if one_dim else fl, nobs)


def assoc_logistic(plink, snps, indiv, Y, covariates=None, spa=False, firth=False, **spa_options):
    """The logistic score test of every SNP for the 0 / 1 traits Y ((indiv, n) or (indiv,), numpy): the null model of each trait is fitted on the host
    (assoc_logistic_null), R, Wt and H are stacked, and assoc_score scans.  Returns AssocScoreResult(score, var, z, nobs) as numpy arrays.  spa=True: the scan
    is assoc_score_spa with P = y - r of every null (spa_options: its z_cutoff, tol, max_iter), and AssocSpaResult(score, var, z, pval, flag, nobs) returns.
    firth=True: the scan is assoc_score_firth (options: its z_cutoff, penalty, tol, max_iter), and AssocFirthResult returns.  Not both."""
    if spa and firth:
        raise ValueError("spa=True and firth=True exclude each other: call assoc_logistic twice")
    Ya = np.asarray(Y, dtype=np.float64)
    one_dim = Ya.ndim == 1
    if Ya.ndim not in (1, 2) or Ya.shape[0] != int(indiv) or (Ya.ndim == 2 and Ya.shape[1] < 1):
        raise ValueError(f"Y needs to be ({indiv},) or ({indiv}, n >= 1): {Ya.shape}")
    if spa_options and not (spa or firth):
        raise ValueError(f"{sorted(spa_options)} need spa=True or firth=True")
    Y2 = Ya.reshape(int(indiv), -1)
    fits = [assoc_logistic_null(Y2[:, c], covariates) for c in range(Y2.shape[1])]
    R = np.asfortranarray(np.stack([f.r for f in fits], axis=1))
    Wt = np.asfortranarray(np.stack([f.w for f in fits], axis=1))
    H = np.asfortranarray(np.concatenate([f.H for f in fits], axis=1))
    if spa:
        res = assoc_score_spa(plink, snps, indiv, np.asfortranarray(Y2 - R), R, Wt, H, **spa_options)
        return AssocSpaResult(*(a.reshape(-1) for a in res[:5]), res.nobs) if one_dim else res
    if firth:
        res = assoc_score_firth(plink, snps, indiv, np.asfortranarray(Y2 - R), R, Wt, H, **spa_options)
        return AssocFirthResult(*(a.reshape(-1) for a in res[:8]), res.nobs) if one_dim else res
    res = assoc_score(plink, snps, indiv, R, Wt, H)
    if one_dim:
        return AssocScoreResult(res.score.reshape(-1), res.var.reshape(-1), res.z.reshape(-1), res.nobs)
    return res


# ---- set tests: burden and SKAT (C entries mxa_assoc_set, mxa_assoc_skat_pvalue)
AssocSetResult = namedtuple("AssocSetResult", "burden burden_var skat c1 c2 c4 burden_p skat_p skat_df phi")
SET_MAX_SIZE = 1024


def assoc_skat_pvalue(Q, c1, c2, c4):
    """(pval, df) of the SKAT statistics Q with the moments c1 = tr A, c2 = tr A^2, c4 = tr A^4, arrays of one shape: Liu's moment matching in its modified form,
    on the host (C entry mxa_assoc_skat_pvalue).  Non-finite or non-positive moments give NaN."""
    q = np.ascontiguousarray(np.asarray(Q, dtype=np.float64))
    m = [np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in (c1, c2, c4)]
    if any(a.shape != q.shape for a in m):
        raise ValueError("Q, c1, c2 and c4 need one shape")
    pval, df = np.zeros(q.shape), np.zeros(q.shape)
    L = _lib.check_library_handle()
    _check(L.mxa_assoc_skat_pvalue(int(q.size), _lib.ptr(q), _lib.ptr(m[0]), _lib.ptr(m[1]), _lib.ptr(m[2]), _lib.ptr(pval), _lib.ptr(df)), "mxa_assoc_skat_pvalue")
    return pval, df


def _set_csr(sets, weights):
    """(set_ptr int64, set_idx int32, set_wt float64 or None).  sets: a LIST of index arrays, or a TUPLE (set_ptr, set_idx) -- the type decides, never the
    contents, so that two index sets are not mistaken for a CSR pair; weights: a list parallel to sets, or flat"""
    if isinstance(sets, tuple):
        if len(sets) != 2 or np.ndim(sets[0]) != 1 or np.ndim(sets[1]) != 1 or len(sets[0]) < 1:
            raise ValueError("a tuple for sets needs to be the CSR pair (set_ptr, set_idx); pass index arrays as a list")
        ptr, idx = np.ascontiguousarray(sets[0], dtype=np.int64), np.ascontiguousarray(sets[1], dtype=np.int32)
        if ptr[0] != 0 or np.any(np.diff(ptr) < 0) or int(ptr[-1]) != idx.size:
            raise ValueError("set_ptr needs to start at 0, not to decrease and to end at len(set_idx)")
    elif isinstance(sets, list):
        arrays = [np.asarray(a, dtype=np.int32).reshape(-1) for a in sets]
        ptr = np.zeros(len(arrays) + 1, dtype=np.int64)
        ptr[1:] = np.cumsum([a.size for a in arrays])
        idx = np.ascontiguousarray(np.concatenate(arrays) if arrays else np.zeros(0, np.int32), dtype=np.int32)
    else:
        raise ValueError("sets needs to be a list of index arrays or the tuple (set_ptr, set_idx)")
    if ptr.size < 2:
        raise ValueError("sets needs to hold at least one set")
    wt = None
    if weights is not None:
        if isinstance(weights, (list, tuple)) and len(weights) and np.ndim(weights[0]) > 0:
            wt = np.concatenate([np.asarray(w, dtype=np.float64).reshape(-1) for w in weights])
        else:
            wt = np.asarray(weights, dtype=np.float64).reshape(-1)
        wt = np.ascontiguousarray(wt, dtype=np.float64)
        if wt.size != idx.size:
            raise ValueError(f"weights need one entry per set entry: {wt.size}, {idx.size}")
    return ptr, idx, wt


def assoc_set(plink, snps, indiv, R, Wt, H, sets, weights=None, out=None, want_phi=False):
    """Burden and SKAT tests of SNP sets under the null models of assoc_score (C entry mxa_assoc_set).  plink, R, Wt, H: as for assoc_score.  sets: a list of
    arrays of SNP indices (any order, overlaps and repeats allowed, at most 1024 each), or the tuple (set_ptr, set_idx) of a CSR list (a list is always index
    arrays, a tuple always the CSR pair); weights: the variant weights omega,
    a list parallel to sets or one flat array parallel to set_idx (None: ones).  Returns AssocSetResult: burden B, burden_var, skat Q, c1, c2, c4, burden_p =
    erfc(|B| / sqrt(2 burden_var)), skat_p and skat_df (assoc_skat_pvalue), each (nsets, n) numpy, or (nsets,) for a one-dimensional R; phi: None, or with
    want_phi=True a list over the sets of (n, m, m) arrays, the null covariance of the set's scores for every trait.  out: an optional dict that receives the
    scan's own "score", "var", "z" ((snps, n) Fortran-ordered numpy, as for assoc_score) and "nobs" ((snps,) int32)."""
    from math import erfc, sqrt
    snps, indiv = int(snps), int(indiv)
    rc, wc, hc, n, kh = _score_operands(plink, snps, indiv, R, Wt, H)
    ptr, idx, wt = _set_csr(sets, weights)
    nsets = ptr.size - 1
    sizes = np.diff(ptr)
    if np.any(sizes < 0) or np.any(sizes > SET_MAX_SIZE) or ptr[0] != 0:
        raise ValueError(f"set sizes need to lie in [0, {SET_MAX_SIZE}]")
    if idx.size and (idx.min() < 0 or idx.max() >= snps):
        raise ValueError(f"set indices need to lie in [0, {snps})")
    one_dim = len(tuple(R.shape)) == 1
    scan = {}
    nobs = None
    if out is not None:
        if any(key not in ("score", "var", "z", "nobs") for key in out):
            raise ValueError("out may hold the keys 'score', 'var', 'z', 'nobs'")
        for key, o in out.items():
            if key == "nobs":
                if not (isinstance(o, np.ndarray) and o.dtype == np.int32 and o.shape == (snps,) and o.flags.c_contiguous):
                    raise ValueError(f"out['nobs'] needs to be a contiguous int32 ({snps},) array")
                nobs = o
                continue
            if not (isinstance(o, np.ndarray) and o.shape == (snps, n) and o.dtype == np.float64 and o.T.flags.c_contiguous):
                raise ValueError(f"out[{key!r}] needs to be a float64 ({snps}, {n}) numpy result with contiguous columns")
            scan[key] = o.T
    stat = np.zeros((6 * n, nsets), dtype=np.float64)
    phi = np.zeros(n * int(np.sum(sizes * sizes)), dtype=np.float64) if want_phi else None
    L = _lib.check_library_handle()
    _check(L.mxa_assoc_set(_lib.ptr(plink), snps, indiv, _lib.ptr(rc), indiv, _lib.ptr(wc), indiv, _lib.ptr(hc), indiv, n, kh, nsets, _lib.ptr(ptr), _lib.ptr(idx),
                           _lib.ptr(wt), _lib.ptr(scan.get("score")), _lib.ptr(scan.get("var")), _lib.ptr(scan.get("z")), snps, _lib.ptr(nobs), _lib.ptr(stat), nsets,
                           _lib.ptr(phi)), "mxa_assoc_set")
    cols = [np.ascontiguousarray(stat[t::6].T) for t in range(6)]          # (nsets, n) each
    with np.errstate(invalid="ignore", divide="ignore"):
        zb = np.abs(cols[0]) / np.sqrt(2.0 * cols[1])
    burden_p = np.array([erfc(v) if np.isfinite(v) else np.nan for v in zb.reshape(-1)]).reshape(zb.shape)
    skat_p, skat_df = assoc_skat_pvalue(cols[2], cols[3], cols[4], cols[5])
    blocks = None
    if want_phi:
        blocks, at = [], 0
        for m in sizes:
            m = int(m)
            blocks.append(phi[at:at + n * m * m].reshape(n, m, m).transpose(0, 2, 1))
            at += n * m * m
    res = cols + [burden_p, skat_p, skat_df]
    if one_dim:
        res = [a.reshape(nsets) for a in res]
    return AssocSetResult(*res, blocks)


def assoc_logistic_sets(plink, snps, indiv, Y, covariates, sets, weights=None, want_phi=False):
    """The set tests for the 0 / 1 traits Y ((indiv, n) or (indiv,), numpy): the null model of each trait is fitted on the host (assoc_logistic_null), R, Wt and H
    are stacked, and assoc_set runs.  Returns AssocSetResult."""
    Ya = np.asarray(Y, dtype=np.float64)
    if Ya.ndim not in (1, 2) or Ya.shape[0] != int(indiv) or (Ya.ndim == 2 and Ya.shape[1] < 1):
        raise ValueError(f"Y needs to be ({indiv},) or ({indiv}, n >= 1): {Ya.shape}")
    Y2 = Ya.reshape(int(indiv), -1)
    fits = [assoc_logistic_null(Y2[:, c], covariates) for c in range(Y2.shape[1])]
    R = np.asfortranarray(np.stack([f.r for f in fits], axis=1))
    Wt = np.asfortranarray(np.stack([f.w for f in fits], axis=1))
    H = np.asfortranarray(np.concatenate([f.H for f in fits], axis=1))
    res = assoc_set(plink, snps, indiv, R, Wt, H, sets, weights, want_phi=want_phi)
    if Ya.ndim == 1:
        return AssocSetResult(*(a.reshape(-1) for a in res[:9]), res.phi)
    return res
