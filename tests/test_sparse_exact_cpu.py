"""CPU: the exact reference of sparse_times_plink (tests/_sparse_ref.py) and the cases tests/test_sparse_exact_gpu.py runs.

1. chain() is the operation: within the first-order bound of a left-to-right fp64 sum of the long-double oracle, and of the reference library's own outputs
   (tests/golden/sparse_golden.npz).  Bound per element: 4 nnz_row 2^-53 sum|a z| (the chain's own forward error is (nnz_row - 1) 2^-53 sum|a z| to first
   order, the reference's sums in groups of 8 stay within the same figure, the long double oracle within 2^-11 of it).
2. The cases discriminate: a chain with a planted fault (_sparse_ref.MUTANTS) differs in bits from chain() wherever the case can show the fault, and a
   wrong order of the additions changes at least a quarter of the outputs of the rows with two or more entries.  These are conditions on the inputs; nothing
   here is measured on the library."""
import os

import numpy as np
import pytest

import _sparse_ref as sr
from _util import Oracle

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_golden.npz")
U = 2.0 ** -53


def magnitude(P, rows, entries, ia, ja, a, ldc):
    """sum |a z| per element, and the stored entries per row, in the layout of chain()"""
    Z = sr.decode(P, rows, entries)
    M = np.zeros((entries, ldc))
    for j in range(len(ia) - 1):
        ts = np.arange(ia[j], ia[j + 1])
        M[:, j] = (np.abs(np.asarray(a)[ts])[:, None] * Z[np.asarray(ja)[ts]]).sum(0)
    nnz = np.zeros(ldc)
    nnz[:len(ia) - 1] = np.diff(ia)
    return M, nnz


def within_bound(C, ref, P, rows, entries, ia, ja, a, ldc):
    M, nnz = magnitude(P, rows, entries, ia, ja, a, ldc)
    return np.all(np.abs(C - ref) <= 4 * nnz[None, :] * U * M)


def differs(x, y):
    return not sr.same_bits(x, y)


@pytest.mark.parametrize("entries, nidx, rows", [(513, 17, 37), (9, 33, 300), (1029, 16, 37), (5, 15, 1)])
def test_chain_agrees_with_the_long_double_oracle(entries, nidx, rows):
    c = sr.tile_case(entries, nidx, rows)
    ldc = nidx + 3
    ref = Oracle().sparse_times_plink(c.P, rows, entries, c.ia, c.ja, c.a, ldc=ldc)
    C = c.want(ldc)
    assert C.shape == ref.shape == (entries, ldc) and np.all(C[:, nidx:] == 0.0) and np.any(C != 0.0)
    assert within_bound(C, ref, c.P, rows, entries, c.ia, c.ja, c.a, ldc)


def test_chain_agrees_with_the_reference_library_outputs():
    g = np.load(GOLD)
    for name in g["names"]:
        snps, indiv, ldc, nidx = (int(x) for x in g[f"{name}/dims"])
        for tc in ("N", "T"):
            P = np.ascontiguousarray(g[f"{name}/plink_t"] if tc == "T" else g[f"{name}/plink"])
            rows, entries = (indiv, snps) if tc == "T" else (snps, indiv)
            ia, ja, a = g[f"{name}/ia{tc}"], g[f"{name}/ja{tc}"], g[f"{name}/a{tc}"]
            C = sr.chain(P, rows, entries, ia, ja, a, ldc=ldc)
            ref = g[f"{name}/C{tc}"]
            assert C.shape == ref.shape and np.all(C[:, nidx:] == 0.0)
            assert within_bound(C, ref, P, rows, entries, ia, ja, a, ldc), (name, tc)


def test_decode_and_pack():
    codes = np.array([[0, 1, 2, 3, 3, 2, 1, 0, 2]], np.uint8)
    P = sr.pack(codes)
    assert P.tolist() == [[0b11100100, 0b00011011, 0b10]]
    assert sr.decode(P, 1, 9).tolist() == [[0, 0, 1, 2, 2, 1, 0, 0, 1]]
    for entries in sr.ENTRIES:
        P = sr.genotypes(37, entries, seed=7)
        c = np.stack([(P >> (2 * q)) & 3 for q in range(4)], axis=-1).reshape(37, -1)
        assert np.all(c[:, entries:] == 0) and np.all(c[:, entries - 1] >= 2)
        if entries >= 511:
            assert abs((c[:, :entries] == 1).mean() - 0.05) < 0.01


def test_the_generator_makes_every_row_shape():
    for nidx, rows in ((17, 37), (33, 300), (16, 37)):
        ia, ja, a = sr.csr_case(nidx, rows, seed=101, long_len=1000 if nidx == 17 else 0)
        n = np.diff(ia)
        per_row = [ja[ia[j]:ia[j + 1]] for j in range(nidx)]
        assert np.any(n == 0) and np.any(n == 1) and np.any((n >= 56) & (n <= 64)) and (nidx != 17 or n.max() >= 1000)
        assert any(len(r) >= 2 and np.any(np.diff(r) < 0) for r in per_row)                       # unsorted
        assert any(len(np.unique(r)) < len(r) for r in per_row)                                   # duplicates within a row
        assert any(len(r) and set(r) <= {0, rows - 1} and len(set(r)) == 2 for r in per_row)      # a row on packed rows 0 and rows - 1 alone
        assert any(len(per_row[i]) and np.array_equal(per_row[i], per_row[j][::-1]) for i in range(nidx) for j in range(i))   # a row's columns again
        assert 0 < len(np.setdiff1d(np.arange(rows), ja)) and 0 in ja and rows - 1 in ja           # packed rows nobody refers to; both ends referred to
        assert np.abs(a).max() <= 2.0 ** 40 and np.abs(a).max() / np.abs(a).min() > 2.0 ** 30


def applicable(c):
    """the planted faults a case can show, decided from its inputs"""
    per_row = [c.ja[c.ia[j]:c.ia[j + 1]] for j in range(c.nidx)]
    out = set()
    if any(len(r) >= 3 for r in per_row):                                # (a sum of two terms is the same in either order)
        out.add("reversed")
    if c.rows > 1 and any(len(r) >= 3 and np.any(np.diff(r) < 0) for r in per_row):
        out.add("sorted")
    if any(len(np.unique(r)) < len(r) for r in per_row):
        out.add("dup_once")
    raw = np.stack([(c.P >> (2 * q)) & 3 for q in range(4)], axis=-1).reshape(c.rows, -1)[:, :c.entries]
    if len(c.ja) and np.any(raw[np.unique(c.ja)] == 1):
        out.add("missing_one")
    if ((c.entries + 3) // 4) % 2:
        out.add("drop_odd_byte")
    if c.entries > sr.SLAB:
        out.add("e_base_ignored")
    return out


def order_fraction(c, mutant):
    """share of the outputs of the rows with two or more entries that a wrong order changes"""
    rows2 = np.flatnonzero(np.diff(c.ia) >= 2)
    a, b = c.want(), c.want(None, mutant)
    return float((a[:, rows2].view(np.uint64) != b[:, rows2].view(np.uint64)).mean()), len(rows2) * c.entries


@pytest.mark.parametrize("entries", sr.ENTRIES)
def test_every_planted_fault_shows_on_the_tile_cases(entries):
    """every case with 15 or more sparse rows shows every fault it can show; a wrong order changes a quarter of the outputs of the rows with two or more
    entries in every such case with more than one packed row and at least 100 of those outputs, and over each entry count as a whole"""
    shown = set()
    changed = {m: [0.0, 0] for m in sr.ORDER_MUTANTS}
    for nidx in sr.NIDX:
        for rows in sr.ROWS:
            c = sr.tile_case(entries, nidx, rows)
            can = applicable(c)
            for m in sorted(can):
                d = differs(c.want(), c.want(None, m))
                if d:
                    shown.add(m)
                assert d or nidx < 15, (entries, nidx, rows, m)
            for m in sr.ORDER_MUTANTS:
                if m in can and nidx >= 15:
                    frac, n = order_fraction(c, m)
                    changed[m][0] += frac * n
                    changed[m][1] += n
                    assert frac >= 0.25 or n < 100 or rows == 1, (entries, nidx, rows, m, frac)      # (one packed row: its zeros blank whole columns)
    want = {"reversed", "sorted", "dup_once"} | ({"missing_one"} if entries >= 2 else set())
    want |= ({"drop_odd_byte"} if ((entries + 3) // 4) % 2 else set()) | ({"e_base_ignored"} if entries > sr.SLAB else set())
    assert shown == want, (entries, shown)
    for m in sr.ORDER_MUTANTS:
        assert changed[m][0] / changed[m][1] >= 0.25, (entries, m, changed[m])


def test_the_one_byte_lane_and_every_slab_are_discriminated():
    """entries 1, 3, 4, 9 and 513 have an odd byte count (the lane with one byte); the slab case shows a slab that reads the first slab's bytes in its second
    and in its third slab; the order faults show on the host-gather case and change 25 % of it"""
    assert [e for e in sr.ENTRIES if ((e + 3) // 4) % 2] == [1, 3, 4, 9, 513]
    c = sr.tile_case(*sr.SLAB_CASE)
    assert c.entries == 2 * sr.SLAB + 5 and c.nidx == 17
    a, b = c.want(c.nidx + 2), c.want(c.nidx + 2, "e_base_ignored")
    assert sr.same_bits(a[:sr.SLAB], b[:sr.SLAB]) and differs(a[sr.SLAB:2 * sr.SLAB], b[sr.SLAB:2 * sr.SLAB]) and differs(a[2 * sr.SLAB:], b[2 * sr.SLAB:])
    for m in sr.ORDER_MUTANTS:
        assert order_fraction(c, m)[0] >= 0.25


def test_the_cases_of_their_own_are_discriminating():
    c = sr.shape_case("single_long")
    assert c.nidx == 1 and c.ia[1] >= 1000 and len(np.unique(c.ja)) < len(c.ja)
    for m in ("reversed", "sorted", "dup_once", "missing_one", "drop_odd_byte", "e_base_ignored"):
        assert differs(c.want(), c.want(None, m)), m
    for name, row in (("first_only", 0), ("last_only", 36)):
        c = sr.shape_case(name)
        assert set(c.ja) == {row} and differs(c.want(), c.want(None, "reversed")) and differs(c.want(), c.want(None, "dup_once"))
    other = sr.chain(np.roll(sr.shape_case("first_only").P, 1, axis=0), 37, 513, *[getattr(sr.shape_case("first_only"), k) for k in ("ia", "ja", "a")])
    assert differs(sr.shape_case("first_only").want(), other)                                   # (another packed row in place of row 0 shows)
    c = sr.shape_case("all_empty")
    assert c.ia[-1] == 0 and not np.any(c.want(c.nidx + 3))
    # inf and NaN: NaN wherever the row with NaN goes; inf or NaN in the row with inf (inf * 0 = NaN where z = 0), finite elsewhere
    c = sr.nonfinite_case()
    C = c.want()
    assert np.all(np.isnan(C[:, 4])) and not np.any(np.isfinite(C[:, 0])) and np.any(np.isinf(C[:, 0])) and np.any(np.isnan(C[:, 0]))
    assert np.all(np.isfinite(np.delete(C, [0, 4], axis=1)))
    # the big case: four non-empty rows around the end of the first launch's row blocks and at the end
    c = sr.big_case()
    n = np.diff(c.ia)
    assert c.nidx == 16 * 65535 + 17 and np.flatnonzero(n).tolist() == [16 * 65535 - 1, 16 * 65535, 16 * 65535 + 1, c.nidx - 1]
    C = c.want(c.nidx + 3)
    assert C.shape == (5, c.nidx + 3) and all(np.any(C[:, j] != 0.0) for j in np.flatnonzero(n)) and differs(C, c.want(c.nidx + 3, "reversed"))
