"""Exact fixtures for the solver twin (potrs_solve_gpu, dcsrtrsv_solve_gpu) and a numpy restatement of the dense schedule of mxa_solve.hip.

Dense family: L = D + N, D diagonal in {1, 2}, N strictly lower with entries in {-1, 0, 1} that are non-zero only at rows in a set R and
columns in a disjoint set C.  Then N D^-1 N = 0, so L^-1 = D^-1 - D^-1 N D^-1 exactly, and M = L L^T has small integer entries.  Every
intermediate of a (blocked, any-order) Cholesky of M is a small dyadic rational: the pivots are 1 or 4, the Schur complements integers, the
inverted diagonal blocks exact.  With X_true integer and B = M X_true a correct solver therefore returns X_true bit for bit, and with
B = I it returns M^-1 = L^-T L^-1 bit for bit.

Sparse family: T triangular, diagonal in {+-0.5, +-1, +-2}, integer off-diagonals in [-2, 2], X_true integer in [-8, 8]: every row of the
substitution is exact in any summation order.
"""
import numpy as np
import scipy.linalg
import scipy.sparse

NB, PANEL = 64, 512        # kPotrfNB, kPotrfPanel of mxa_solve.hip
DGEMM_BN = 128             # column tile of k_dgemm (the right-hand sides of the solve products)


def exact_factor(n, seed, per_row=12):
    """Sparse L = D + N of the exact family (CSR) and the diagonal d.  Row 0 is in C and row n-1 in R, so the last row always couples back."""
    rng = np.random.default_rng(seed)
    d = rng.choice([1.0, 2.0], n)
    in_r = rng.random(n) < 0.5
    in_r[0] = False
    if n > 1:
        in_r[-1] = True
    rows = np.repeat(np.flatnonzero(in_r), per_row)
    cols = np.floor(rng.random(rows.size) * rows).astype(np.int64)     # uniform in [0, row)
    keep = ~in_r[cols]
    key = np.unique(rows[keep] * n + cols[keep])
    rows, cols = key // n, key % n
    vals = rng.choice([-1.0, 1.0], rows.size)
    Lsp = scipy.sparse.csr_matrix((np.concatenate([d, vals]), (np.concatenate([np.arange(n), rows]), np.concatenate([np.arange(n), cols]))), shape=(n, n))
    return Lsp, d


def exact_spd(n, seed, per_row=12):
    """(M dense, L dense, d) of the exact family; M = L L^T formed as a sparse product of integers (exact)."""
    Lsp, d = exact_factor(n, seed, per_row)
    M = (Lsp @ Lsp.T).toarray()
    return M, Lsp.toarray(), d


def exact_inverse_factor(L, d):
    """L^-1 = D^-1 - D^-1 N D^-1, exactly (dyadic entries of magnitude at most 1)."""
    N = np.tril(L, -1)
    Di = 1.0 / d
    return np.diag(Di) - Di[:, None] * N * Di[None, :]


def exact_logdet(d):
    return 2.0 * np.log(2.0) * np.count_nonzero(d == 2.0)


def exact_rhs(M, nrhs, seed):
    """X_true integer in [-4, 4] and B = M X_true (exact: small integers)."""
    X = np.random.default_rng(seed).integers(-4, 5, size=(M.shape[0], nrhs)).astype(np.float64)
    return X, M @ X


def blocked_cholesky_solve(M, B, fault=None):
    """numpy restatement of dense_solve_impl (mxa_solve.hip): 64-column diagonal blocks factored and inverted, the block column below as a
    product with the inverted block, the rest of the 512-column panel updated per block; after each panel L(p) (the next panel's columns) and
    B(p) (everything right of it); then the two triangular solves block by block through the inverted blocks.  Reads only the lower
    triangle of M.  `fault` plants one defect:
      'skip_far_small'   B(p) is skipped when 0 < far <= 128 (a lower_only update of one tile)
      'skip_next_small'  L(p) is skipped when fewer than 128 rows trail the panel
      'rhs_first_tile'   the solve products only touch the first 128 right-hand sides (a k_dgemm without column tiles beyond blockIdx.y = 0)
    Returns (X, logdet)."""
    n = M.shape[0]
    A = np.tril(M).astype(np.float64)
    inv = []
    for K in range(0, n, PANEL):
        pw = min(PANEL, n - K)
        for k in range(K, K + pw, NB):
            nb = min(NB, K + pw - k)
            L11 = np.linalg.cholesky(A[k:k + nb, k:k + nb])
            Li = scipy.linalg.solve_triangular(L11, np.eye(nb), lower=True)
            A[k:k + nb, k:k + nb] = L11
            inv.append(Li)
            if k + nb < n:
                A[k + nb:, k:k + nb] = A[k + nb:, k:k + nb] @ Li.T
                rest = K + pw - k - nb
                if rest > 0:
                    A[k + nb:, k + nb:K + pw] -= A[k + nb:, k:k + nb] @ A[k + nb:K + pw, k:k + nb].T
        trailing = n - K - pw
        if trailing <= 0:
            break
        pw1 = min(PANEL, trailing)
        P21 = A[K + pw:, K:K + pw]
        if not (fault == "skip_next_small" and trailing < 128):
            A[K + pw:, K + pw:K + pw + pw1] -= P21 @ P21[:pw1].T
        far = trailing - pw1
        if far > 0 and not (fault == "skip_far_small" and far <= 128):
            P31 = P21[pw1:]
            A[K + pw + pw1:, K + pw + pw1:] -= P31 @ P31.T
    X = np.array(B, dtype=np.float64, copy=True)
    cols = slice(0, DGEMM_BN) if fault == "rhs_first_tile" else slice(None)
    nblk = len(inv)
    for kb in range(nblk):
        off = kb * NB
        nb = min(NB, n - off)
        X[off:off + nb, cols] = inv[kb] @ X[off:off + nb, cols]
        if off + nb < n:
            X[off + nb:, cols] -= A[off + nb:, off:off + nb] @ X[off:off + nb, cols]
    for kb in range(nblk - 1, -1, -1):
        off = kb * NB
        nb = min(NB, n - off)
        X[off:off + nb, cols] = inv[kb].T @ X[off:off + nb, cols]
        if off > 0:
            X[:off, cols] -= A[off:off + nb, :off].T @ X[off:off + nb, cols]
    return X, float(np.sum(2.0 * np.log(np.diag(A))))


def exact_triangular(m, seed, structure, lower):
    """Sparse triangular T (CSR) of the exact sparse family.  structure: 'random' (a few entries per row, some rows long), 'band' (the 200
    sub/super-diagonals), 'full' (the whole triangle)."""
    rng = np.random.default_rng(seed)
    diag = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], m)
    if structure == "full":
        r, c = np.tril_indices(m, -1)
    elif structure == "band":
        r = np.concatenate([np.arange(o, m) for o in range(1, min(m, 201))] + [np.zeros(0, np.int64)])
        c = r - np.concatenate([np.full(m - o, o) for o in range(1, min(m, 201))] + [np.zeros(0, np.int64)])
    else:
        cnt = rng.integers(0, 9, m)
        cnt[rng.random(m) < 0.05] = 150                                 # some rows with more than 64 off-diagonal entries
        r = np.repeat(np.arange(m), cnt)
        c = np.floor(rng.random(r.size) * r).astype(np.int64)
        keep = r > 0
        key = np.unique(r[keep] * m + c[keep])
        r, c = key // m, key % m
    v = rng.integers(-2, 3, r.size).astype(np.float64)
    v[v == 0] = 1.0
    T = scipy.sparse.csr_matrix((np.concatenate([diag, v]), (np.concatenate([np.arange(m), r]), np.concatenate([np.arange(m), c]))), shape=(m, m))
    return T if lower else T.T.tocsr()
