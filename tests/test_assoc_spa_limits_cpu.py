"""The inputs of tests/test_assoc_spa_limits_gpu.py without a device: every case passes the conditions under which the device may be compared with the two
references of tests/_assoc_spa_ref.py (equal flags in float64 and long double, no |z| within 2^-40 z_cutoff of the cutoff, no support margin within
[2^-31, 2^-29] A, at most 20 evaluations a side), and the builders put the marks where the kernels change path.  Only the host null model of the library runs.

Seen with the library's own null model (x86-64, 80-bit long double), flags as [0, 1, 2, 3]:
  lists       (67, 700, 3, 1, z 0.5): 577 marked SNPs, 1145 items, eps 2.5e-14, 10 evaluations at most; (259, 300, 8, 2, z 1): 269 marked SNPs, 716 items, eps
              1.3e-14, 12 evaluations; (259, 33, 3, 10, z 1): 21 marked SNPs, 30 items, eps 1.9e-15
  pool        (67, 130, 2, 1, z 1.5): 33 loud rows (5 with two marks, 28 with one), 97 quiet rows, no flag 2 or 3 but the appended missing row
  max_iter    (259, 300, 8, 2, z 1): flag 1 / flag 2 = 7 / 709 (max_iter 4), 609 / 107 (6), 705 / 11 (8); float64 and long double at tol 2^-30 need the same
              number of evaluations on every item
  tol 2^-12   (259, 130, 3, 3, z 2): equal flags and evaluation counts, eps 5.9e-15
  tail        the six rows of TAIL_ROWS: flag 1, at most 12 evaluations; 1027: p from 1e-14 down to 1e-67; 4099: down to 7e-290; 8195: four rows at exactly 0"""
import os

import numpy as np
import pytest

import _assoc_spa_ref as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#        MXA_ASSOC_SPA_ITEMS, MXA_ASSOC_SPA_BATCH (None: unset), what ends a batch before the last on (67, 700, 3, 1, z 0.5).  Nine SNPs hold at least nine items
#        and three SNPs at most nine, so of the two mixed pairs the first is cut by the items alone and the second by the rows alone; (4, 3) is cut by both.
KNOBS = [(1, None, {"items"}), (4, None, {"items"}), (7, None, {"items"}), (1000, None, {"items"}), (7, 9, {"items"}), (1000, 3, {"rows"}), (4, 3, {"items", "rows"})]


def rounds(flags):
    """(marked SNPs, items) of each 256-SNP round of the device's compaction"""
    cnt = (np.asarray(flags) == 1).sum(axis=1)
    return [(int((cnt[s:s + 256] > 0).sum()), int(cnt[s:s + 256].sum())) for s in range(0, len(cnt), 256)]


@pytest.mark.parametrize("indiv, snps, n, kh, z_cutoff, marked_above", [c + (m,) for c, m in zip(sp.LIST_CASES, (512, 256, 0))])
def test_the_list_cases_meet_the_conditions_and_mark_enough_snps(indiv, snps, n, kh, z_cutoff, marked_above):
    ref = sp.limits_reference(indiv, snps, n, kh, z_cutoff)
    per_round = rounds(ref["flags"])
    marked, items = sum(r[0] for r in per_round), sum(r[1] for r in per_round)
    print(f"indiv {indiv} snps {snps} n {n} kh {kh} z_cutoff {z_cutoff}: flags {np.bincount(ref['flags'].ravel(), minlength=4)}, {marked} marked SNPs, {items} items, "
          f"per round {per_round}, eps {ref['eps']:.3g}, evaluations {max(ref['e64'].max(), ref['eld'].max())}")
    assert marked > marked_above and items > marked and ref["eps"] <= 2.0 ** -40
    assert max(ref["e64"].max(), ref["eld"].max()) <= 12
    if marked_above == 0:
        assert n * (kh + 2) > 32
    else:
        assert len(per_round) >= 2 and all(r[0] > 0 for r in per_round)          # every round of the list hands its counts on to the next
        assert items > 512                                                       # the unbatched run: three blocks of k_assoc_spa_combine


def test_the_pool_has_loud_and_quiet_rows_of_every_kind():
    pool = sp.pool()
    flags = pool["ref"]["flags"]
    two, one, quiet, missing = pool["two"], pool["one"], pool["quiet"], pool["missing"]
    print(f"pool: flags {np.bincount(flags.ravel(), minlength=4)}, {len(two)} rows with two marks, {len(one)} with one, {len(quiet)} quiet, eps {pool['ref']['eps']:.3g}")
    assert len(two) >= 1 and len(one) >= 1 and len(two) + len(one) >= 4 and len(quiet) >= 4
    assert np.all(flags[two] == 1) and np.all((flags[one] == 1).sum(axis=1) == 1) and np.all(flags[one] <= 1) and np.all(flags[quiet] == 0)
    assert np.all(flags[missing] == 3) and np.all(np.isnan(pool["ref"]["p64"][missing])) and not np.any(flags[:missing] >= 2)
    assert np.all(pool["codes"][missing] == -1)


def test_the_layouts_put_the_marks_on_the_round_boundaries():
    pool = sp.pool()
    flags = pool["ref"]["flags"]
    lay = pool["layouts"]
    assert sorted(lay) == ["all_loud", "alternating", "edges", "empty_and_full"]
    marked = {}
    for name, rows in lay.items():
        assert rows.shape == (sp.ROUNDS_TOTAL,) and rows.min() >= 0 and rows.max() <= pool["missing"]
        f = flags[rows]
        cnt = (f == 1).sum(axis=1)
        marked[name] = np.flatnonzero(cnt > 0)
        # two-item and one-item SNPs in turn along the marked positions
        assert np.array_equal(cnt[marked[name]], np.where(np.arange(len(marked[name])) % 2 == 0, 2, 1)), name
        assert np.all(f[cnt == 0] != 2)
        print(f"{name}: {len(marked[name])} marked SNPs, {int(cnt.sum())} items, per round {rounds(f)}")
    assert list(marked["edges"]) == [0, 255, 256, 511, 512, 1029]
    assert list(np.flatnonzero((flags[lay["edges"]] == 3).all(axis=1))) == [254, 768]
    assert list(marked["empty_and_full"]) == list(range(256, 512)) + [1029]
    assert [r[0] for r in rounds(flags[lay["empty_and_full"]])] == [0, 256, 0, 0, 1]
    assert [r[0] for r in rounds(flags[lay["all_loud"]])] == [256, 256, 256, 256, 6]
    assert list(marked["alternating"]) == list(range(1, 1030, 2)) and np.all(np.diff(marked["alternating"]) > 1)
    for name in ("empty_and_full", "all_loud", "alternating"):
        assert not np.any(flags[lay[name]] == 3)
    # the reference of a layout is the pool's, indexed: a SNP's result does not depend on the other rows
    P, R, Wt, H = pool["operands"]
    rows = lay["edges"][250:260]
    p64, f64, _, _, _ = sp.spa_reference(pool["codes"][rows], P, R, Wt, H, pool["z_cutoff"])
    assert np.array_equal(f64, flags[rows]) and np.array_equal(p64.view(np.int64), pool["ref"]["p64"][rows].view(np.int64))


@pytest.mark.parametrize("which", ["list", "edges"])
def test_the_item_knob_cuts_where_the_table_says(which):
    if which == "list":
        n, flags = 3, sp.limits_reference(*sp.LIST_CASES[0])["flags"]
    else:
        pool = sp.pool()
        n, flags = 2, pool["ref"]["flags"][pool["layouts"]["edges"]]
    off = sp.item_offsets(flags)
    nk = len(off) - 1
    assert sp.batch_cuts(off, 1 << 40, nk) == [(0, nk, "end")]
    for items, rows, want in KNOBS:
        cuts = sp.batch_cuts(off, max(n, items), rows or nk)
        why = {c[2] for c in cuts[:-1]}
        print(f"{which}: MXA_ASSOC_SPA_ITEMS {items}, MXA_ASSOC_SPA_BATCH {rows}: {len(cuts)} batches, ended by {sorted(why)}")
        assert cuts[0][0] == 0 and cuts[-1][1] == nk and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
        assert all(off[k1] - off[k0] <= max(n, items) and k1 - k0 <= (rows or nk) for k0, k1, _ in cuts)
        if which == "list":
            assert why == want, (items, rows, why)
        elif rows is None and items < off[nk]:
            assert why == {"items"}
        if items == 1:                                  # raised to n: a SNP with all n traits marked still goes in one batch
            assert max(off[k1] - off[k0] for k0, k1, _ in cuts) == n
        # batches that do not start on a multiple of the tile of k_assoc_spa_form
        assert which == "edges" or any(k0 % 8 for k0, _, _ in cuts)


def test_the_item_knob_is_read_per_call_and_documented():
    read = lambda *parts: open(os.path.join(ROOT, *parts)).read()          # noqa: E731
    source = read("miraculix_amd", "csrc", "mxa_assoc_spa.hip")
    body = source[source.index("long spa_batch_items("):source.index("long spa_batch_rows(")]
    assert 'getenv("MXA_ASSOC_SPA_ITEMS")' in body and "static" not in body and "std::max<long>(n," in body
    header = read("include", "miraculix_amd.h")
    comment = header[header.index("The score test with saddlepoint p-values"):header.index("int mxa_assoc_score_spa(")]
    assert "MXA_ASSOC_SPA_ITEMS" in comment and comment.index("MXA_ASSOC_SPA_BATCH") < comment.index("MXA_ASSOC_SPA_ITEMS")
    design = read("DESIGN.md")
    at = design.index("`MXA_ASSOC_SPA_BATCH`")
    assert "`MXA_ASSOC_SPA_ITEMS`" in design[at:at + 200]


def test_max_iter_between_4_and_8_fails_some_sides_and_solves_others():
    indiv, snps, n, kh, z_cutoff = sp.MAX_ITER_CASE
    codes, _, _, _, P, R, Wt, H = sp.limits_operands(indiv, snps, n, kh)
    ref = sp.limits_reference(indiv, snps, n, kh, z_cutoff)
    # the same number of evaluations in float64 and in long double at the entry's stop rule: rounding decides no flag
    _, fld, _, eld, _ = sp.spa_reference(codes, P, R, Wt, H, z_cutoff, 2.0 ** -30, 50, sp.LD)
    assert np.array_equal(fld, ref["flags"]) and np.array_equal(eld, ref["e64"])
    assert not np.any(ref["flags"] >= 2)
    for max_iter in (4, 6, 8):
        p, f, z, e, _ = sp.spa_reference(codes, P, R, Wt, H, z_cutoff, 2.0 ** -30, max_iter, np.float64)
        ones, twos = int((f == 1).sum()), int((f == 2).sum())
        print(f"max_iter {max_iter}: flag 1 {ones}, flag 2 {twos}")
        assert ones >= 5 and twos >= 5 and ones + twos == (ref["flags"] == 1).sum()
        assert np.array_equal(f == 2, (ref["flags"] == 1) & (ref["e64"] > max_iter))
        assert all(p[s, c] == sp.normal_p(z[s, c]) for s, c in np.argwhere(f == 2))
        assert np.array_equal(p[f == 1].view(np.int64), ref["p64"][f == 1].view(np.int64))


def test_a_loose_tolerance_stops_both_references_at_the_same_evaluation():
    indiv, snps, n, kh, z_cutoff = sp.LOOSE_TOL_CASE
    ref = sp.limits_reference(indiv, snps, n, kh, z_cutoff, sp.LOOSE_TOL, sp.LOOSE_TOL)
    tight = sp.limits_reference(indiv, snps, n, kh, z_cutoff)
    print(f"tol 2^-12: flags {np.bincount(ref['flags'].ravel(), minlength=4)}, eps {ref['eps']:.3g}, evaluations {ref['e64'].max()} (tol 2^-30: {tight['e64'].max()})")
    assert np.array_equal(ref["e64"], ref["eld"]) and (ref["flags"] == 1).sum() >= 5 and ref["eps"] <= 2.0 ** -40
    # the tolerance decides something: fewer evaluations, and p-values the tight run does not give
    assert ref["e64"].sum() < tight["e64"].sum() and np.array_equal(ref["flags"], tight["flags"])
    on = ref["flags"] == 1
    assert np.any(ref["p64"][on] != tight["p64"][on])


@pytest.mark.parametrize("indiv", sp.TAIL_INDIV)
def test_the_tail_rows_reach_down_to_the_underflow_of_erfc(indiv):
    codes, _, Y, _, P, R, Wt, H = sp.tail_operands(indiv)
    ref = sp.tail_reference(indiv)
    rows = len(sp.TAIL_ROWS)
    p64, pld = ref["p64"][:rows, 0], ref["pld"][:rows, 0]
    print(f"indiv {indiv}: {int(Y.sum())} cases, flags {np.bincount(ref['flags'].ravel(), minlength=4)}, p of the six rows {[float(f'{v:.3g}') for v in p64]}, "
          f"eps_rel {ref['eps_rel']:.3g}, evaluations {max(ref['e64'].max(), ref['eld'].max())}")
    assert not np.any(codes[:rows] < 0) and np.all(ref["flags"][:rows] == 1)
    assert max(ref["e64"][:rows].max(), ref["eld"][:rows].max()) <= 12
    assert np.all(np.isfinite(p64)) and np.all(p64 >= 0) and p64.max() < 1e-10
    assert ref["eps_rel"] <= 2.0 ** -40
    if indiv == 1027:
        assert p64.min() > 1e-200
    if indiv == 4099:
        assert 0 < p64.min() < 1e-200 and np.all(pld > sp.TAIL_FLOOR)
    if indiv == 8195:
        # (the long-double reference takes its erfc from the double one and a first-order term: below the underflow it is that term alone, some 1e-336)
        assert (p64 == 0).sum() >= 2 and np.all(np.abs(pld[p64 == 0]) < 1e-300) and np.any((p64 > 0) & (p64 < 1e-100))


def test_the_tail_rule_refuses_what_it_should():
    ref = sp.tail_reference(8195)
    p64, pld = ref["p64"], ref["pld"]
    assert sp.tail_errors(p64, p64, pld) == ref["eps_rel"]
    zero, deep = np.argwhere(p64 == 0)[0], np.argwhere((p64 > 0) & (p64 < 1e-100))[0]
    for at, value in ((zero, 1e-299), (zero, -0.5), (zero, np.nan), (deep, 0.0)):
        bad = p64.copy()
        bad[tuple(at)] = value
        with pytest.raises(AssertionError):
            sp.tail_errors(bad, p64, pld)
    off = p64.copy()
    off[tuple(deep)] *= 1 + 1e-9                       # 1e-9 in log p over |log p| of some hundreds: above 16 eps_rel
    assert sp.tail_errors(off, p64, pld) > 16 * max(ref["eps_rel"], 2.0 ** -48)
