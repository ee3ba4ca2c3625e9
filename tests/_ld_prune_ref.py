"""The greedy selection of mxa_ld_prune_csr / mxa_ld_window_prune(_pairwise), restated as the sequential walk of its definition; shared by the prune tests.

G: the strict upper CSR (rowptr, col) read as an undirected graph.  a comes before b iff priority[a] < priority[b], or the priorities are equal and a < b
(priority None: a < b).  Walk the SNPs in that order; keep a SNP iff none of its neighbours has been kept.  owner[v] = v for a kept v, else the first kept
neighbour of v in the order."""
import numpy as np


def order_of(snps, priority):
    """the SNPs in the order of the walk (-0.0 and 0.0 compare equal: the index decides)"""
    if priority is None:
        return np.arange(snps)
    return np.lexsort((np.arange(snps), np.asarray(priority, dtype=np.float64)))


def neighbours(snps, rowptr, col):
    """(start, nb): the neighbours of v, both triangles, are nb[start[v]: start[v + 1]]"""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    rows = np.repeat(np.arange(snps, dtype=np.int64), np.diff(rowptr))
    a, b = np.concatenate([rows, col]), np.concatenate([col, rows])
    o = np.argsort(a, kind="stable")
    return np.concatenate([[0], np.cumsum(np.bincount(a, minlength=snps))]).astype(np.int64), b[o]


def ref_greedy(snps, rowptr, col, priority):
    """(keep bool, owner int32) by the sequential walk"""
    start, nb = neighbours(snps, rowptr, col)
    order = order_of(snps, priority)
    rank = np.empty(snps, dtype=np.int64)
    rank[order] = np.arange(snps)
    keep, owner = np.zeros(snps, dtype=bool), np.full(snps, -1, dtype=np.int32)
    for v in order:
        n = nb[start[v]: start[v + 1]]
        kept = n[keep[n]]                                                                # every one of them comes before v: a later SNP is still unvisited
        if kept.size == 0:
            keep[v], owner[v] = True, v
        else:
            owner[v] = kept[np.argmin(rank[kept])]
    return keep, owner


def csr_of_edges(snps, edges):
    """(rowptr int64, col int32) of the strict upper triangle from a list of pairs in any orientation"""
    e = sorted({(min(a, b), max(a, b)) for a, b in edges})
    assert all(0 <= a < b < snps for a, b in e)
    rows = np.array([a for a, _ in e], dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=snps))]).astype(np.int64)
    return rowptr, np.array([b for _, b in e], dtype=np.int32)
