"""The closed forms of tests/_ld_limits_ref.py held to the brute-force helpers, on the CPU at about 1000 SNPs with the windows scaled down: the rows against
_ld_apply_ref.dense / _ld_op_ref.windowed, the banded product against W @ X, the prune results against _ld_prune_ref's sequential walk on the whole graph."""
import numpy as np
import pytest
import torch

import _ld_apply_ref as ar
import _ld_limits_ref as lim
import _ld_op_ref as opr
import _ld_ref as ref

BANDS = [(1003, 1, lim.B1_COEF), (1003, 63, lim.C1_COEF), (997, 130, lim.C1_COEF), (5, 1, lim.B1_COEF), (40, 2047, lim.C1_COEF), (1, 1, lim.B1_COEF)]


def _dense_closed_form(snps, w, coef):
    """W[i, j] from the definition, element by element: V[min, |i - j|] inside the band, 0 outside"""
    a, b = coef
    W = np.zeros((snps, snps))
    for i in range(snps):
        for j in range(i, min(i + w, snps - 1) + 1):
            W[i, j] = W[j, i] = 1.0 if i == j else ((a * i + b * (j - i)) % 17 - 8) / 8.0
    return W


@pytest.mark.parametrize("snps,w,coef", BANDS)
def test_banded_rows_and_product_against_the_dense_matrix(snps, w, coef):
    last = lim.band_last(snps, w).numpy()
    assert np.array_equal(last, ref.fixed_last(snps, w)) and last.dtype == np.int32
    rows = lim.band_rows(snps, w, coef, chunk_rows=97).numpy()            # several chunks of the rectangular part
    assert np.array_equal(rows, lim.band_rows(snps, w, coef).numpy())
    entries, mirrored = lim.band_entries(snps, w)
    assert entries == len(rows) == int(ref.rowptr_of(last)[-1])
    first = ref.first_of(last)
    assert mirrored == int((last - first + 1).sum())
    W = opr.windowed(ar.dense(rows, last), last)
    assert np.array_equal(W, _dense_closed_form(snps, w, coef))
    assert np.all(np.abs(W * 8) == np.round(np.abs(W * 8))) and np.abs(W).max() <= 1.0      # multiples of 1 / 8
    for n in (1, 3):
        X = lim.band_x(snps, n)
        Xn = X.numpy().T
        assert np.array_equal(Xn, (7 * np.arange(snps)[:, None] + 3 * np.arange(n)[None, :]) % 9 - 4.0)
        for shift in (0.0, 0.5, 2.0):
            Y = lim.band_apply(snps, w, coef, X, shift).numpy().T
            assert np.array_equal(Y, opr.apply_exact(W, Xn, shift)), (n, shift)
            exact = W.astype(np.longdouble) @ Xn.astype(np.longdouble) + np.longdouble(shift) * Xn
            assert np.array_equal(Y.astype(np.longdouble), exact), (n, shift)                # the float64 sums are exact


def test_entry_counts_of_the_large_cases():
    assert lim.band_entries(1_100_000, 2047) == (2_250_703_872, 4_500_307_744)
    assert lim.band_entries((1 << 24) + 300, 1) == (2 * ((1 << 24) + 300) - 1, 3 * ((1 << 24) + 300) - 2)
    assert lim.b2_marks((1 << 26) + 5) == [1 << 25, 1 << 26]


def test_relres_is_the_column_norm_quotient():
    B = torch.tensor([[3.0, 4.0], [1.0, 0.0]], dtype=torch.float64)
    R = torch.tensor([[0.0, 5e-10], [1e-12, 0.0]], dtype=torch.float64)
    assert np.allclose(lim.relres(B, R), [1e-10, 1e-12], rtol=1e-15)


@pytest.mark.parametrize("snps", (1005, 64, 11))
@pytest.mark.parametrize("reverse", (False, True))
def test_sparse_prune_expectation_against_the_walk_on_the_whole_graph(snps, reverse):
    from _ld_prune_ref import csr_of_edges, ref_greedy
    edges = lim.b2_edges(snps)
    touched, keep_t, owner_t, n_kept = lim.sparse_prune_expected(snps, edges, reverse)
    rowptr, col = csr_of_edges(snps, edges)
    rp, cl = lim.sparse_csr(snps, edges)
    assert np.array_equal(rp.numpy(), rowptr) and np.array_equal(cl.numpy(), col) and rp.dtype == torch.int64 and cl.dtype == torch.int32
    keep, owner = ref_greedy(snps, rowptr, col, -np.arange(snps, dtype=np.float64) if reverse else None)
    want_keep, want_owner = np.ones(snps, bool), np.arange(snps)
    want_keep[touched], want_owner[touched] = keep_t, owner_t
    assert np.array_equal(keep, want_keep) and np.array_equal(owner, want_owner) and n_kept == int(keep.sum())
    assert 0 < (~keep).sum() < len(touched)


@pytest.mark.parametrize("snps,w", [(1000, 127), (1000, 31), (129, 127), (128, 127), (5, 7)])
@pytest.mark.parametrize("reverse", (False, True))
def test_full_window_prune_closed_form_against_the_walk(snps, w, reverse):
    from _ld_prune_ref import ref_greedy
    rowptr, col = lim.full_window_csr(snps, w)
    assert rowptr[-1] == len(col) == int(ref.rowptr_of(ref.fixed_last(snps, w))[-1]) - snps
    keep, owner = ref_greedy(snps, rowptr, col, -np.arange(snps, dtype=np.float64) if reverse else None)
    k, o, n_kept = lim.full_window_prune_expected(snps, w, reverse)
    assert k.dtype == torch.uint8 and o.dtype == torch.int32
    assert np.array_equal(k.numpy().astype(bool), keep) and np.array_equal(o.numpy(), owner) and n_kept == int(keep.sum())


def test_the_large_full_window_case_keeps_four():
    assert lim.full_window_prune_expected(lim.BIG_SNPS, lim.BIG_W, False)[2] == 4
    assert lim.full_window_prune_expected(lim.BIG_SNPS, lim.BIG_W, True)[2] == 4
