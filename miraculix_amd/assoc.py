"""Association scan (C entries mxa_assoc_basis, mxa_assoc_linear): per-SNP linear regression y ~ 1 + covariates + x_s on packed genotypes, missing calls
imputed by the SNP's mean.  The definition, the operation order and what is exact: include/miraculix_amd.h."""
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
