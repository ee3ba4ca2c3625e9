"""The inputs of tests/test_assoc_firth_limits_gpu.py without a device: every case reaches the branch of the Newton loop of mxa_assoc_score_firth that it is
for, in the float64 AND in the long-double reference of tests/_assoc_firth_ref.py, whose `fit` now records a trace (the decisions of every evaluation).  So the
device file excludes nothing, and no decision of the loop hangs on a rounding that the device may do differently.  Only the host null model of the library runs.

Seen (x86-64, 80-bit long double; flags as [0, 1, 2, 3], without / with the penalty):
  bisect      the 22 rows of BISECT_ROWS among 33, 24 (259) and 25 (1027) fitted items, kh 1: 8 / 14 items (259) and 12 / 14 (1027) bisect twice, 2 / 2 and
              6 / 6 never, 8 and 7 of the bisecting items have U < 0; kh 3 at 259: 16 / 16.  The nearest a Newton beta' comes to the bracket end it is compared with
              is 3e-4 |beta'|.  At most 12 evaluations.  (`edge` is the distance to the bracket end that is NOT beta itself: to the end at beta the distance is the
              step, which the stop rule has just found above tol |beta'| and which is 1e-9 ... 1e-5 |beta'| on the last step but one of every converging item.)
  alt         penalty 1: 4 of the 6 items of ALT_ROWS have an evaluation with alt <= 0; |alt| >= 0.056 K'' everywhere; penalty 0 solves all six
  negative    U < 0: rows 0-2 OUTSIDE without the penalty (margin exactly 0) and solved with beta < 0 with it; rows 3-5 solved with margin / A 2.1e-3 ... 2.8e-3
              (259), 5.2e-4 ... 9.3e-4 (1027)
  saturated   rows 0-7 FAILED at evaluation 2 with max |beta g| >= 2.3e4, rows 8-11 at evaluation 1 (beta = 0), both penalties; flags [10, 2, 12, 0] (259) and
              [0, 12, 12, 0] (1027)
  zero        (67, n 1): 9 cells with U == 0 exactly, 8 more with |z| < 0.05, flags [0, 31, 0, 2]; (259, n 3): 19 and 14, flags [0, 91, 2, 6] / [0, 93, 0, 6].  The
              chisq before max(0, .) is exactly 0 on the cells with U == 0 and positive on every other: NO seed tried (1 ... 5 in place of LIMITS_SEED) gave a
              negative one, so the clamp `fmax(x2, 0.0)` is NOT reached by these tests.
  tails       p-values of the six rows: 1e-14 ... 6e-68 (1027), 1e-60 ... 3.5e-290 (4099), 1e-120, 1e-250 and four times exactly 0 (8195)
  lists       (67, 700, 3, 1, z 0.5): 1145 items with either penalty
  max_iter    bisect_operands(259) at z_cutoff 0.25 and tol 2^-6: flag 1 / flag 2 = 3 / 28, 6 / 25, 20 / 11 (max_iter 2, 4, 6; penalty 0) and 3 / 28, 9 / 22, 26 / 5
              (penalty 1); 22 of the items that fail at max_iter 2 fail on an evaluation that bisected"""
import math

import numpy as np
import pytest

import _assoc_firth_ref as fr
from test_assoc_spa_limits_cpu import KNOBS

FAR = 2.0 ** -20


def items(ref):
    """(cell, float64 trace, long-double trace) of every item"""
    return [(a["cell"], a, b) for a, b in zip(ref["t64"], ref["tld"])]


def same_decisions(a, b):
    """bisected or not, evaluation by evaluation, equal in two traces.  The long-double run stops at a tighter tolerance, so it may evaluate further; where one
    of the two has stopped the other must not bisect any more"""
    k = min(len(a["bisected"]), len(b["bisected"])) - 1
    return a["bisected"][:k] == b["bisected"][:k] and not any(a["bisected"][k:]) and not any(b["bisected"][k:])


def counts(ref):
    return np.bincount(ref["flags"].ravel(), minlength=4)


def test_a_trace_changes_no_result():
    codes, _, _, _, P, R, Wt, H = fr.bisect_operands(259)
    for penalty in (0, 1):
        trace = []
        plain, traced = fr.firth_reference(codes, P, R, Wt, H, 1.0, penalty), fr.firth_reference(codes, P, R, Wt, H, 1.0, penalty, trace=trace)
        for key in ("beta", "se", "chisq", "pval", "z", "flag", "evals"):
            assert np.array_equal(plain[key], traced[key], equal_nan=True), key
        assert len(trace) == int((plain["flag"] != 0).sum()) and [t["evals"] for t in trace] == [plain["evals"][t["cell"]] for t in trace]
        assert all(len(t[k]) == t["evals"] for t in trace for k in ("beta", "replaced", "ratio", "bisected", "edge", "reach"))


@pytest.mark.parametrize("penalty", [0, 1])
@pytest.mark.parametrize("indiv, kh", [(259, 1), (1027, 1), (259, 3)])
def test_bisect_rows_take_the_bisection_on_both_sides_and_far_from_the_bracket(indiv, kh, penalty):
    ref = fr.limits_reference("bisect", (indiv, kh), penalty)
    flags = ref["flags"]
    fitted = [(cell, a, b) for cell, a, b in items(ref) if flags[cell] == 1]
    twice = sum(1 for _, a, _ in fitted if sum(a["bisected"]) >= 2)
    never = sum(1 for _, a, _ in fitted if not any(a["bisected"]))
    negative = sum(1 for _, a, _ in fitted if a["U"] < 0 and any(a["bisected"]))
    edges = [e for _, a, b in fitted for t in (a, b) for e in t["edge"] if not math.isnan(e)]
    print(f"bisect indiv {indiv} kh {kh} penalty {penalty}: flags {counts(ref)}, {twice} items bisect twice or more, {never} never, {negative} with U < 0 bisect, "
          f"nearest to the far end of the bracket {min(edges):.3g}, eps {ref['eps']:.3g}, evaluations {ref['r64']['evals'].max()} / {ref['rld']['evals'].max()}")
    assert twice >= 6 and never >= 1 and negative >= 1
    assert all(same_decisions(a, b) for _, a, b in fitted)
    assert all(sum(a["bisected"]) == sum(b["bisected"]) for _, a, b in fitted)
    # beta' = beta - f / f' with f' > 0 lies on the inner side of the bracket end that the sign of f has just moved to beta, by the step the stop rule has
    # just found larger than tol |beta'|; `edge` is its distance to the other end, the one the comparison can fail at
    assert min(edges) >= FAR
    assert not np.any(flags >= 2)


@pytest.mark.parametrize("indiv", fr.LIMITS_INDIV)
def test_alt_rows_reach_a_penalised_slope_that_is_not_positive(indiv):
    rows = len(fr.ALT_ROWS)
    ref = fr.limits_reference("alt", (indiv,), 1)
    for which in ("t64", "tld"):
        special = [t for t in ref[which] if t["cell"][0] < rows]
        replaced = sum(1 for t in special if any(t["replaced"]))
        ratios = np.array([r for t in ref[which] for r in t["ratio"]])
        print(f"alt indiv {indiv} ({which}): flags {counts(ref)}, {replaced} of {len(special)} rows with alt <= 0 at {sum(sum(t['replaced']) for t in special)} evaluations, "
              f"min |alt| / K'' {np.abs(ratios).min():.3g}, eps {ref['eps']:.3g}")
        assert replaced >= 3 and np.all(np.abs(ratios) >= FAR)
        assert all(t["replaced"] == [r <= 0 for r in t["ratio"]] for t in ref[which])
    assert all(a["replaced"][:len(b["replaced"])] == b["replaced"][:len(a["replaced"])] for _, a, b in items(ref))
    assert np.all(ref["flags"][:rows] == 1)
    plain = fr.limits_reference("alt", (indiv,), 0)
    assert np.all(plain["flags"][:rows] == 1) and not any(any(t["replaced"]) for t in plain["t64"] + plain["tld"])
    codes = fr.alt_operands(indiv)[0]
    assert not np.any(codes[:rows] < 0) and [((codes[r] == 1).sum(), (codes[r] == 2).sum()) for r in range(rows)] == fr.ALT_ROWS


@pytest.mark.parametrize("indiv", fr.LIMITS_INDIV)
def test_negative_rows_cover_the_three_outcomes_of_the_support_test(indiv):
    plain, pen = fr.limits_reference("negative", (indiv,), 0), fr.limits_reference("negative", (indiv,), 1)
    by_cell = {w: {cell: (a, b) for cell, a, b in items(r)} for w, r in (("plain", plain), ("pen", pen))}
    assert np.all(plain["r64"]["z"][:9] < -fr.NEG_CUTOFF)
    margins = []
    for row in range(9):
        for a in by_cell["plain"][(row, 0)] + by_cell["pen"][(row, 0)]:
            assert a["U"] < 0
    for row in (0, 1, 2):                      # carried by controls alone
        a, b = by_cell["plain"][(row, 0)]
        assert a["status"] == b["status"] == fr.OUTSIDE and a["margin"] == b["margin"] == 0 and plain["flags"][row, 0] == 2
        assert pen["flags"][row, 0] == 1 and pen["rld"]["beta"][row, 0] < 0 and pen["r64"]["beta"][row, 0] < 0
    for row in (3, 4, 5):                      # one case allele among hundreds
        a, b = by_cell["plain"][(row, 0)]
        assert a["status"] == b["status"] == fr.SOLVED and plain["flags"][row, 0] == 1 and 1e-4 <= a["margin"] <= 1e-2 and 1e-4 <= b["margin"] <= 1e-2
        margins.append(a["margin"])
        assert pen["flags"][row, 0] == 1 and pen["rld"]["beta"][row, 0] < 0
    m = np.array(plain["rld"]["margins"])
    assert not np.any((m >= 2.0 ** -31) & (m <= 2.0 ** -29))
    print(f"negative indiv {indiv}: flags {counts(plain)} / {counts(pen)}, margins / A of rows 3-5 {[float(f'{v:.3g}') for v in margins]}, eps {plain['eps']:.3g} / "
          f"{pen['eps']:.3g}")


@pytest.mark.parametrize("penalty", [0, 1])
@pytest.mark.parametrize("indiv", fr.LIMITS_INDIV)
def test_saturated_rows_fail_at_the_first_or_second_evaluation_beside_solved_items(indiv, penalty):
    ref = fr.limits_reference("saturated", (indiv,), penalty)
    by_cell = {cell: (a, b) for cell, a, b in items(ref)}
    signs = set()
    for row in range(2 * len(fr.SAT_ZONES)):
        at = 2 if row < 8 else 1
        for t in by_cell[(row, 0)]:
            assert t["status"] == fr.FAILED and t["evals"] == at and t["beta"][0] == 0, (row, t)
            assert all(r <= 600 or r >= 800 for r in t["reach"]), t["reach"]
            assert (t["reach"][-1] >= 800) == (at == 2)
            signs.add((at, t["U"] > 0))
        assert ref["flags"][row, 0] == 2 and abs(ref["r64"]["z"][row, 0]) >= fr.SAT_CUTOFF
    assert signs == {(1, False), (1, True), (2, False), (2, True)}
    reach = [r for t in ref["t64"] + ref["tld"] for r in t["reach"]]
    assert all(r <= 600 or r >= 800 for r in reach)
    # solved items in the same list, before and behind: the failed ones are the first items of their trait
    assert (ref["flags"][2 * len(fr.SAT_ZONES):] == 1).sum() >= 2 and not np.any(ref["flags"][2 * len(fr.SAT_ZONES):] >= 2)
    codes, _, _, _, P, R, Wt, H = fr.saturated_operands(indiv)
    assert not np.any(codes[:, :fr.SAT_KEEP_OUT][2 * len(fr.SAT_ZONES):] != 0) and np.all(Wt > 0) and set(P[80:120, 0]) == {0.0, 1.0}
    print(f"saturated indiv {indiv} penalty {penalty}: flags {counts(ref)}, largest |beta g| {max(reach):.3g}, eps {ref['eps']:.3g}")


@pytest.mark.parametrize("penalty", [0, 1])
@pytest.mark.parametrize("indiv, n", fr.ZERO_CASES)
def test_a_zero_cutoff_fits_every_finite_cell_and_those_with_a_score_of_exactly_zero(indiv, n, penalty):
    """The clamp max(0, chisq) is not reached: the chisq before it is exactly 0 where U == 0 and positive elsewhere (see the module's docstring)."""
    ref = fr.limits_reference("zero", (indiv, n), penalty)
    codes, _, Y, _, P, R, Wt, H = fr.zero_operands(indiv, n)
    z64, zld, flags = ref["r64"]["z"], ref["rld"]["z"], ref["flags"]
    exact = (z64 == 0) & (zld == 0)
    assert np.array_equal(z64 == 0, zld == 0) and exact.sum() >= 3 and np.all(P == 0.5) and H.shape[1] == 0
    small = (np.abs(z64) < 0.05) & ~exact
    assert small.sum() >= 3 and np.all(flags[0] == 3) and np.all(flags[1] == 3) and not np.any(flags == 0)
    assert np.array_equal(flags == 3, ~np.isfinite(z64))
    for s, c in np.argwhere(exact):
        assert not np.any(codes[s] < 0) and codes[s][Y[:, c] > 0].sum() == codes[s][Y[:, c] == 0].sum() > 0       # as many alleles in cases as in controls
        assert flags[s, c] == 1 and ref["r64"]["evals"][s, c] == 1 and ref["rld"]["evals"][s, c] == 1
        for r in (ref["r64"], ref["rld"]):
            assert r["beta"][s, c] == 0 and r["chisq"][s, c] == 0 and r["pval"][s, c] == 1 and r["se"][s, c] > 0
    raw = {w: np.array([float(t["chisq"]) for t in ref[w] if t["chisq"] is not None]) for w in ("t64", "tld")}
    print(f"zero cutoff indiv {indiv} n {n} penalty {penalty}: flags {counts(ref)}, {int(exact.sum())} cells with U == 0, {int(small.sum())} more with |z| < 0.05, "
          f"chisq before the clamp >= {raw['t64'].min():.3g} / {raw['tld'].min():.3g} ({int((raw['t64'] < 0).sum())} negative), eps {ref['eps']:.3g}")
    assert np.abs(raw["t64"]).min() <= 1e-12 and np.abs(raw["tld"]).min() <= 1e-12
    assert (raw["t64"] == 0).sum() == exact.sum() and not np.any(raw["t64"] < 0) and not np.any(raw["tld"] < 0)


def test_the_measures_with_a_reference_of_zero_refuse_what_they_should():
    ref = fr.limits_reference("zero", (67, 1), 1)
    r64, rld, on = ref["r64"], ref["rld"], ref["flags"] == 1
    assert max(fr.limit_errors(r64, rld, on).values()) == ref["eps"] <= 2.0 ** -40
    at = tuple(np.argwhere((rld["beta"] == 0) & on)[0])
    bound = 16 * max(ref["eps"], 2.0 ** -48)
    for key, value, caught in (("beta", 1e-9, True), ("beta", 1e-18, False), ("chisq", 1e-9, True), ("chisq", 1e-18, False), ("pval", 1 - 1e-9, True), ("se", 0.0, True)):
        bad = {k: np.array(v, dtype=np.float64) for k, v in r64.items() if k in ("beta", "se", "chisq", "pval")}
        bad[key][at] = value
        assert (max(fr.limit_errors(bad, rld, on).values()) > bound) == caught, (key, value)
    bad["chisq"][at] = -1e-18
    with pytest.raises(AssertionError):
        fr.limit_errors(bad, rld, on)
    # where neither holds a zero the measures are those of errors()
    other = fr.limits_reference("bisect", (259, 1), 1)
    assert fr.limit_errors(other["r64"], other["rld"], other["flags"] == 1) == fr.errors(other["r64"], other["rld"], other["flags"] == 1)


def test_the_tail_rows_span_1e_14_to_the_underflow_of_erfc():
    rows = len(fr.TAIL_ROWS)
    seen = []
    for indiv in fr.LIMITS_TAIL_INDIV:
        for penalty in (0, 1):
            ref = fr.limits_reference("tail", (indiv,), penalty)
            p64, pld = ref["r64"]["pval"][:rows, 0], ref["rld"]["pval"][:rows, 0]
            eps_rel = fr.tail_errors(ref["r64"]["pval"], ref["r64"]["pval"], ref["rld"]["pval"])
            print(f"tail indiv {indiv} penalty {penalty}: flags {counts(ref)}, p of the six rows {[float(f'{v:.3g}') for v in p64]}, eps {ref['eps']:.3g}, eps_rel {eps_rel:.3g}, "
                  f"evaluations {ref['r64']['evals'].max()} / {ref['rld']['evals'].max()}")
            assert np.all(ref["flags"][:rows] == 1) and np.all(np.isfinite(p64)) and np.all(p64 >= 0) and p64.max() < 1e-10 and eps_rel <= 2.0 ** -40
            assert not np.any(ref["flags"] >= 2)
            if indiv == 8195:
                assert (p64 == 0).sum() >= 2 and np.all(np.abs(pld[p64 == 0]) < 1e-300) and np.any((p64 > 0) & (p64 < 1e-100))
            seen.extend(p64)
    seen = np.array(seen)
    assert seen.max() >= 1e-15 and seen.min() < 1e-290 and seen[seen > 0].min() < 1e-280 and np.any((seen > 1e-200) & (seen < 1e-100))


@pytest.mark.parametrize("penalty", [0, 1])
def test_the_long_list_holds_more_items_than_one_launch_of_the_fit_keeps_resident(penalty):
    ref = fr.limits_reference("list", (0,), penalty)
    marked = ref["flags"] != 0
    assert np.isin(ref["flags"], (0, 1, 2)).all() and marked.sum() > 1024
    off = fr.item_offsets(marked.astype(np.int32))
    nk, n = len(off) - 1, 3
    assert off[nk] == marked.sum()
    ends = set()
    for knob_items, knob_rows, want in KNOBS:
        cuts = fr.batch_cuts(off, max(n, knob_items), knob_rows or nk)
        why = {c[2] for c in cuts[:-1]}
        assert why == want, (knob_items, knob_rows, why)
        ends |= {tuple(sorted(why))}
    assert ends == {("items",), ("rows",), ("items", "rows")}
    print(f"list penalty {penalty}: flags {counts(ref)}, {nk} marked SNPs, {int(off[nk])} items, eps {ref['eps']:.3g}")
    for index in (1, 2):
        other = fr.limits_reference("list", (index,), penalty)
        assert (other["flags"] == 1).sum() >= 30 and other["eps"] <= 2.0 ** -38


@pytest.mark.parametrize("penalty", [0, 1])
def test_max_iter_2_4_6_fails_some_items_and_solves_others_and_rounding_decides_no_flag(penalty):
    full, _ = fr.max_iter_flags(penalty, 50)
    in_bisection = 0
    for max_iter in fr.MAX_ITERS:
        flags, trace = fr.max_iter_flags(penalty, max_iter)
        ones, twos = int((flags == 1).sum()), int((flags == 2).sum())
        failed_bisecting = sum(1 for t in trace if t["status"] == fr.FAILED and t["evals"] == max_iter and t["bisected"][-1])
        print(f"max_iter {max_iter} penalty {penalty}: flag 1 {ones}, flag 2 {twos}, {failed_bisecting} failed on an evaluation that bisected")
        assert ones >= 3 and twos >= 3 and ones + twos == ((full == 1) | (full == 2)).sum()
        in_bisection += failed_bisecting
        assert np.array_equal(flags, fr.max_iter_flags(penalty, max_iter, fr.LD)[0])
        for factor in (0.99, 1.01):
            assert np.array_equal(flags, fr.max_iter_flags(penalty, max_iter, np.float64, factor)[0]), factor
    assert in_bisection >= 1


@pytest.mark.parametrize("penalty", [0, 1])
@pytest.mark.parametrize("indiv", fr.LIMITS_INDIV)
@pytest.mark.parametrize("tol", fr.LIMITS_TOLS)
def test_the_flags_at_a_loose_and_a_tight_tolerance_do_not_hang_on_the_tolerance(indiv, tol, penalty):
    codes, _, _, _, P, R, Wt, H = fr.bisect_operands(indiv)
    flags = [fr.firth_reference(codes, P, R, Wt, H, fr.BISECT_CUTOFF, penalty, t, 50)["flag"] for t in (tol, 0.5 * tol, 2 * tol)]
    assert np.array_equal(flags[0], flags[1]) and np.array_equal(flags[0], flags[2]) and (flags[0] == 1).sum() >= 20
    loose = tol > 2.0 ** -30
    ref = fr.limits_reference("bisect", (indiv, 1), penalty, tol, tol if loose else fr.TOL_LD)
    tight = fr.limits_reference("bisect", (indiv, 1), penalty)
    assert np.array_equal(ref["flags"], flags[0]) and np.array_equal(ref["flags"], tight["flags"])
    e, et = ref["r64"]["evals"], tight["r64"]["evals"]
    print(f"tol 2^{round(math.log2(tol))} indiv {indiv} penalty {penalty}: flags {counts(ref)}, eps {ref['eps']:.3g}, evaluations {e.max()} (tol 2^-30: {et.max()})")
    if loose:                                  # both references stop at the same evaluation, earlier than at 2^-30: the comparison on the device means something
        assert np.array_equal(e, ref["rld"]["evals"]) and e.sum() < et.sum() and ref["eps"] <= 2.0 ** -36
        on = ref["flags"] == 1
        assert np.any(ref["r64"]["beta"][on] != tight["r64"]["beta"][on])
    else:
        assert e.sum() >= et.sum() and np.all(e >= et)
