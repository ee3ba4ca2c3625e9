"""Closed forms of the limit tests of the LD pairs / prune / apply / operator entries (tests/test_ld_limits_gpu.py): plain numpy and torch, nothing of the
library is imported.  Every function that builds a large operand takes a torch device, so the GPU tests build on the device and tests/test_ld_limits_cpu.py
holds the same code, on the CPU and at small sizes, to the brute-force helpers (_ld_op_ref.windowed, _ld_apply_ref.dense, W @ X, _ld_prune_ref.ref_greedy).

The banded family (the operator at 2^24 + 300 SNPs: w = 1; with 4.5 10^9 mirrored entries: w = 2047).  Upper ragged rows with the window last[i] = min(i + w, snps - 1):
    V[i, 0] = 1,  V[i, d] = ((A i + B d) mod 17 - 8) / 8  for d = 1 .. last[i] - i          (A, B) = (1, 0) at w = 1, (5, 3) at w = 2047
    X[i, c] = ((7 i + 3 c) mod 9) - 4
Every value is a multiple of 1 / 8 of magnitude <= 1, X a small integer, shift in {0, 0.5, 2}: every product and partial sum of
    Y[i, c] = shift X[i, c] + sum_{d = 0 .. w, i + d < snps} V[i, d] X[i + d, c] + sum_{d = 1 .. w, i - d >= 0} V[i - d, d] X[i - d, c]
is a multiple of 1 / 16 far below 2^53, i.e. exact in float64 in any order: the apply is compared for equality.

The prune graphs.  Sparse: a handful of edges around the marks (the rows at which a row sweep of four rows per workgroup starts a new piece of 2^23 or 2^24
workgroups) and a path on the last three rows; expected results by _ld_prune_ref's sequential walk on the touched vertices alone, relabelled 0 .. k - 1 in
index order -- an untouched vertex has no neighbour, is kept and owns itself.  Full window w (every pair i < j <= i + w is an edge): in index order
the walk keeps 0, removes 1 .. w, keeps w + 1, ..: keep[i] = (i mod (w + 1) == 0), owner[v] = v - v mod (w + 1); under priority[i] = -i the mirror image."""
import numpy as np
import torch

from _ld_prune_ref import csr_of_edges, ref_greedy

B1_COEF, C1_COEF = (1, 0), (5, 3)


# ------------------------------------------------------------------------------------------------------------------------------ banded family
def band_last(snps, w, device="cpu"):
    return torch.clamp(torch.arange(snps, dtype=torch.int32, device=device) + w, max=snps - 1)


def band_entries(snps, w):
    """stored entries of the upper ragged rows, and of the mirrored rows the operator keeps"""
    w = min(w, snps - 1)
    entries = snps * (w + 1) - w * (w + 1) // 2
    return entries, 2 * entries - snps


def _v(i, d, coef):
    """V[i, d] for integer tensors i, d (broadcast), float64"""
    a, b = coef
    off = (((a * i + b * d) % 17) - 8).to(torch.float64) / 8.0
    return torch.where(d == 0, torch.ones_like(off), off)


def band_rows(snps, w, coef, device="cpu", chunk_rows=None):
    """the upper ragged rows, row i = V[i, 0 .. last[i] - i]: the rectangular part (rows of w + 1 entries) in chunks of rows (2^25 entries: the temporaries
    stay below 2 GB), then the ragged tail"""
    w = min(w, snps - 1)
    entries, _ = band_entries(snps, w)
    chunk_rows = chunk_rows or max(1, (1 << 25) // (w + 1))
    rows = torch.empty(entries, dtype=torch.float64, device=device)
    nrect = snps - w                                                    # rows 0 .. nrect - 1 hold w + 1 entries
    d = torch.arange(w + 1, dtype=torch.int64, device=device)[None, :]
    for i0 in range(0, nrect, chunk_rows):
        i1 = min(nrect, i0 + chunk_rows)
        i = torch.arange(i0, i1, dtype=torch.int64, device=device)[:, None]
        rows[i0 * (w + 1): i1 * (w + 1)] = _v(i, d, coef).reshape(-1)
    if w:
        ln = torch.arange(w, 0, -1, dtype=torch.int64, device=device)   # the lengths of rows nrect .. snps - 1
        ti = torch.repeat_interleave(torch.arange(nrect, snps, dtype=torch.int64, device=device), ln)
        start = torch.cumsum(ln, 0) - ln
        td = torch.arange(int(ln.sum()), dtype=torch.int64, device=device) - torch.repeat_interleave(start, ln)
        rows[nrect * (w + 1):] = _v(ti, td, coef)
    return rows


def band_x(snps, n, device="cpu"):
    """X as n contiguous columns (an n x snps tensor: column-major snps x n with ld = snps)"""
    i = torch.arange(snps, dtype=torch.int64, device=device)[None, :]
    c = torch.arange(n, dtype=torch.int64, device=device)[:, None]
    return (((7 * i + 3 * c) % 9) - 4).to(torch.float64)


def band_apply(snps, w, coef, X, shift):
    """Y (n x snps) of the docstring's closed form: a loop over d of two shifted vector FMAs in float64"""
    w = min(w, snps - 1)
    Y = (1.0 + shift) * X                                               # d = 0: the diagonal is 1
    i = torch.arange(snps, dtype=torch.int64, device=X.device)
    for d in range(1, w + 1):
        v = _v(i[: snps - d], torch.full((), d, dtype=torch.int64, device=X.device), coef)[None, :]      # V[i, d], i = 0 .. snps - d - 1
        Y[:, : snps - d].addcmul_(v, X[:, d:])                          # row i takes V[i, d] X[i + d]
        Y[:, d:].addcmul_(v, X[:, : snps - d])                          # row i + d takes V[i, d] X[i]
    return Y


def relres(B, R):
    """|R|_2 / |B|_2 per column (rows of the n x snps tensors)"""
    return (torch.linalg.vector_norm(R, dim=1) / torch.linalg.vector_norm(B, dim=1)).cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------- the prune graphs
def b2_marks(snps):
    """the rows at which a piece of 2^23 or 2^24 workgroups of four rows would start, below snps - 5; at small sizes (the CPU test) two marks inside"""
    marks = [m for m in (4 << 23, 4 << 24) if m + 1 < snps - 3]
    return marks if marks else [snps // 3, (2 * snps) // 3]


def b2_edges(snps):
    """paths m - 1, m, m + 1 around every mark, a path on the last three rows, and one long edge from row 0 to the first mark"""
    e = []
    for m in b2_marks(snps):
        e += [(m - 1, m), (m, m + 1)]
    e += [(snps - 3, snps - 2), (snps - 2, snps - 1), (0, b2_marks(snps)[0])]
    return e


def sparse_prune_expected(snps, edges, reverse):
    """(touched vertices ascending, keep there, owner there, n_kept) by the sequential walk on the touched vertices; reverse: priority[i] = -i"""
    touched = np.array(sorted({v for e in edges for v in e}), dtype=np.int64)
    small = {int(v): k for k, v in enumerate(touched)}
    rowptr, col = csr_of_edges(len(touched), [(small[a], small[b]) for a, b in edges])
    keep, owner = ref_greedy(len(touched), rowptr, col, -np.arange(len(touched), dtype=np.float64) if reverse else None)
    return touched, keep, touched[owner], snps - int((~keep).sum())


def sparse_csr(snps, edges, device="cpu"):
    """(rowptr int64 of snps + 1, col int32) of the strict upper triangle, rowptr built on the device"""
    e = sorted({(min(a, b), max(a, b)) for a, b in edges})
    cnt = torch.zeros(snps + 1, dtype=torch.int64, device=device)
    rows = torch.tensor([a for a, _ in e], dtype=torch.int64, device=device)
    cnt.index_add_(0, rows + 1, torch.ones_like(rows))
    return torch.cumsum(cnt, 0), torch.tensor([b for _, b in e], dtype=torch.int32, device=device)


def full_window_prune_expected(snps, w, reverse, device="cpu"):
    """(keep uint8, owner int32, n_kept) of the graph of every pair i < j <= i + w"""
    i = torch.arange(snps, dtype=torch.int64, device=device)
    if reverse:
        m = (snps - 1 - i) % (w + 1)
        keep, owner = m == 0, i + m
    else:
        m = i % (w + 1)
        keep, owner = m == 0, i - m
    return keep.to(torch.uint8), owner.to(torch.int32), (snps + w) // (w + 1)


def full_window_csr(snps, w):
    """numpy (rowptr, col) of the full-window graph (the CPU test's size)"""
    last = np.minimum(np.arange(snps) + w, snps - 1)
    rowptr = np.concatenate([[0], np.cumsum(last - np.arange(snps))]).astype(np.int64)
    col = np.concatenate([np.arange(i + 1, last[i] + 1) for i in range(snps)]).astype(np.int32)
    return rowptr, col


# ------------------------------------------------------------------------------------------------------ the data of the tests with > 2^31 stored entries
BIG_SNPS, BIG_INDIV, BIG_W = 100_000, 64, 32_767


def big_window_problem():
    """The problem of test_ld_window_edges_gpu.py::test_more_than_two_to_the_31_stored_entries, shared with the pairs / prune / apply tests at that size:
    100 000 x 64 seeded binomial genotypes with no monomorphic SNP, the fixed window w = 32 767 (2 739 945 472 stored entries), and 10^5 sampled flat
    positions k of the ragged rows, half of them above 2^31, 64 in the last row and the rows before it; (si, sj) the pair of position k.  rng: the generator
    after these draws (the caller's further draws continue the sequence)."""
    import _ld_ref as ref
    from _util import pack_plink
    snps, indiv, w = BIG_SNPS, BIG_INDIV, BIG_W
    rng = np.random.default_rng([snps, indiv])
    Z = rng.binomial(2, rng.uniform(0.05, 0.95, size=snps)[:, None], size=(snps, indiv)).astype(np.int8)
    const = Z.min(axis=1) == Z.max(axis=1)
    Z[const, 0], Z[const, 1] = 0, 2
    X = np.ascontiguousarray(pack_plink(Z))
    assert np.array_equal(ref.staged(X[:50])[:, :indiv], Z[:50])
    Zl = Z.astype(np.int64)
    f = Zl.sum(axis=1) / (2.0 * indiv)
    diag = (Zl * Zl).sum(axis=1)
    assert np.all(diag - 4.0 * indiv * f * f > 0)
    last = ref.fixed_last(snps, w)
    rowptr = ref.rowptr_of(last)
    total = int(rowptr[-1])
    assert total == 2_739_945_472 and total > 2 ** 31
    k = np.concatenate([rng.integers(0, 2 ** 31, size=50_000), rng.integers(2 ** 31, total, size=49_936), np.arange(total - 64, total)])
    si = np.searchsorted(rowptr, k, side="right") - 1
    sj = si + (k - rowptr[si])
    assert np.all(sj <= last[si]) and (k > 2 ** 31).sum() * 3 >= len(k) and (si == snps - 1).any() and len(k) == 100_000
    return dict(snps=snps, indiv=indiv, w=w, X=X, Zl=Zl, f=f, diag=diag, last=last, rowptr=rowptr, total=total, k=k, si=si, sj=sj, rng=rng)
