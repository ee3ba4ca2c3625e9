"""mxa_assoc_score_firth where its Newton loop, tails and lists had never run (tests/test_assoc_firth_gpu.py: case fraction 0.03-0.07, at most 300 SNPs, tol
2^-30, max_iter in {1, 3, 50}, p > 1e-200, cutoffs >= 1).  The cases, their references and the traces of the loop are built in tests/_assoc_firth_ref.py;
tests/test_assoc_firth_limits_cpu.py asserts without a device that every case takes the branch it is for, in float64 and in long double alike.  One
comparison (`compare`) is used everywhere: flags equal to the float64 reference's; score, var, z and nobs bit for bit mxa_assoc_score's; the cells with the
flags 0, 2 and 3 exactly the one-step values or NaN (check_unfitted_cells); over the fitted cells beta and se (relative; where the reference's |beta| < 2^-20 se:
|d beta| / se), chisq / max(1, chisq) and log pval within 16 max(eps, 2^-48) of the long-double reference, eps = the two references' largest difference over
that case's fitted cells; in the tail cases log pval by the relative rule of tail_errors (tests/_assoc_spa_ref.py) with its rules for the underflow; host and
device operands give the same bits.

What each test reaches in mxa_assoc_spa.hip that the suite had not (spa_newton_step is the safeguarded step that k_assoc_firth shares with k_assoc_spa):
  bisect        spa_newton_step: `if (!(tn > lo && tn < hi)) tn = 0.5 * (lo + hi)` taken once to three times an item, on both sides (`if (f < 0.0) lo = t; else
                hi = t` with both ends finite), beside items of the same launch that never take it; kh 3: the same with g != 0 at every individual.
  alt           k_assoc_firth: `if (alt > 0.0) fp = alt` NOT taken (alt <= 0, K'' stands in) at one evaluation of four items.
  negative      k_assoc_firth: the support test on U < 0, `-((v4[3] - c0) - U)`: kSpaOutside written (penalty 0, margin exactly 0), passed with a margin of
                5e-4 ... 3e-3 A, and skipped with the penalty (beta^ < 0).
  saturated     spa_newton_step: `if (!isfinite(tn)) return kNewtonFailed` at the first evaluation (K''(0) = 0) and at the second (every exp(-|beta g|) = 0: f / 0
                without the penalty, 0 / 0 with it); k_assoc_firth_combine: `if (a.status != kSpaSolved) return` beside solved items of the same batch.
  zero cutoff   k_assoc_firth_classify: `az < z_cutoff` with z_cutoff = 0 (false for z = 0); k_assoc_firth: f = 0 exactly, tn = t = 0 accepted at the first
                evaluation by `fabs(tn - t) <= tol * fabs(tn)` (spa_newton_step) with both sides 0; k_assoc_firth_combine: x2 = 0, pval = erfc(0) = 1.  (`fmax(x2, 0.0)` is not
                reached with a negative x2: tests/test_assoc_firth_limits_cpu.py.)
  tails         k_assoc_firth_combine: `erfc(sqrt(0.5 * x2))` from 1e-14 down to 3.5e-290 and past its underflow (x2 up to 2700); k_assoc_firth with 33
                individuals a thread (8195).
  lists         spa_stage with firth: 1145 items, more than kFirthResident = 1024 workgroups of k_assoc_firth in one launch; k_assoc_firth_combine with
                blockIdx.x > 0; the batches cut by items, by rows and by both, item_base = off[k0] > 0 in both kernels.
  max_iter      spa_newton_step: `evals >= max_iter` on an evaluation that bisected, and on one that did not, beside accepted items.
  tol           spa_newton_step: the stop rule at 2^-12 (an evaluation or two earlier) and 2^-40 (later).

Measured on an MI355X (flags as [0, 1, 2, 3]; eps seen on x86-64 with 80-bit long double / the device's largest of the four differences; penalty 0, then 1):
  bisect (259, kh 1)        flags [9, 24, 0, 0]: 6.4e-14 / 1.9e-14 and 6.2e-14 / 2.4e-14
  bisect (1027, kh 1)       flags [8, 25, 0, 0]: 9.1e-13 / 1.3e-13 and 9.1e-13 / 1.3e-13
  bisect (259, kh 3)        flags [9, 24, 0, 0]: 1.1e-14 / 7.5e-15 and 1.4e-14 / 1.0e-14
  alt (259)                 flags [0, 24, 0, 0]: 1.4e-14 / 1.5e-14 and 2.3e-14 / 2.0e-14
  alt (1027)                flags [0, 24, 0, 0]: 5.2e-14 / 5.5e-14 and 6.8e-14 / 4.9e-14
  negative (259)            flags [6, 15, 3, 0] and [6, 18, 0, 0]: 2.5e-14 / 1.9e-14 and 2.1e-14 / 1.6e-14
  negative (1027)           flags [8, 13, 3, 0] and [8, 16, 0, 0]: 5.3e-13 / 6.8e-14 and 4.3e-13 / 5.1e-14
  zero cutoff (67, n 1)     flags [0, 31, 0, 2]: 1.0e-13 / 2.3e-14 and 2.3e-14 / 4.3e-14; 9 cells with U = 0: beta = 0, chisq = 0, pval = 1 exactly
  zero cutoff (259, n 3)    flags [0, 91, 2, 6] and [0, 93, 0, 6]: 1.9e-13 / 1.2e-12 and 2.1e-13 / 2.1e-13; 19 cells with U = 0
  saturated (259)           flags [10, 2, 12, 0]: 4.6e-15 / 3.6e-15 and 5.3e-15 / 7.3e-15
  saturated (1027)          flags [0, 12, 12, 0]: 4.0e-14 / 5.7e-14 and 3.6e-14 / 3.9e-14
  (67, 700, 3, 1, z 0.5)    1145 items, flags [955, 1145, 0, 0]: 5.4e-14 / 1.5e-14 and 1.4e-12 / 2.0e-12
  (259, 300, 8, 2, z 1)     716 items, flags [1684, 716, 0, 0]: 9.1e-15 / 3.1e-14 and 8.2e-15 / 2.9e-14
  (259, 33, 3, 10, z 1)     30 items, flags [69, 30, 0, 0]: 4.0e-15 / 5.5e-15 and 3.5e-15 / 5.0e-15
  max_iter on bisect (259) at z_cutoff 0.25, tol 2^-6    flags [2, 3, 28, 0] (max_iter 2), [2, 6, 25, 0] (4), [2, 20, 11, 0] (6) and [2, 3, 28, 0], [2, 9, 22, 0],
                            [2, 26, 5, 0]: the references' own, and the accepted cells carry the bits of the uncapped run
  tol 2^-12 on bisect       259: 5.4e-14 / 2.1e-14 and 3.3e-14 / 2.3e-14; 1027: 1.0e-12 / 1.5e-13 and 1.0e-12 / 9.0e-14
  tol 2^-40 on bisect       259: 6.4e-14 / 1.9e-14 and 7.4e-14 / 1.8e-14; 1027: 9.1e-13 / 1.3e-13 and 9.1e-13 / 1.4e-13
  the tail (eps / the device's largest difference in beta, se and chisq; eps_rel / the device's largest |log pval - log p_LD| / max(1, |log p_LD|); log10
  pval of the six rows without the penalty):
    1027    flags [10, 14, 0, 0]: 6.8e-14 / 9.1e-14, 4.7e-14 / 6.1e-14 and 1.5e-13 / 5.2e-14, 1.1e-13 / 3.5e-14; -67.2, -62.5, -30.5, -13.9, -59.1, -48.5
    4099    flags [12, 12, 0, 0]: 1.9e-13 / 1.6e-13, 1.4e-13 / 1.1e-13 and 1.9e-13 / 3.3e-13, 1.3e-13 / 2.3e-13; -289.5, -270.0, -126.6, -60.0, -253.5, -202.7
    8195    flags [15, 9, 0, 0]: 3.4e-13 / 6.2e-13, 2.4e-13 / 4.2e-13 and 3.3e-13 / 1.9e-13, 2.2e-13 / 1.3e-13; 0, 0, -250.0, -120.1, 0, 0 (exactly 0 with the flag 1
            where erfc underflows)
  Every figure lies below its bound 16 max(eps, 2^-48); the device disagreed with the references nowhere.
"""
import math

import numpy as np
import pytest

import _assoc_firth_ref as fr
import _operands as op
from test_assoc_firth_gpu import MAX_ITER, TOL, check_unfitted_cells, run, run_score, same
from test_assoc_spa_limits_gpu import KNOBS

pytestmark = pytest.mark.gpu

FIT = ("beta", "se", "chisq", "pval")


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


def compare(mx, label, operands, z_cutoff, penalty, ref, tail=False, tol=TOL, max_iter=MAX_ITER):
    """the comparison of the module's docstring on one call with host operands, then the same call with device operands: the same bits.  Returns the host
    call's result."""
    plink, P, R, Wt, H = operands
    rld, flags, eps = ref["rld"], ref["flags"], ref["eps"]
    got = run(mx, plink, P, R, Wt, H, z_cutoff, penalty, tol, max_iter)
    (score, var, z), nobs = run_score(mx, plink, R, Wt, H)
    for name, want in (("score", score), ("var", var), ("z", z), ("nobs", nobs)):
        assert np.array_equal(op.bits(got[name]), op.bits(want)), name
    assert np.array_equal(got["flag"], flags), (np.argwhere(got["flag"] != flags)[:5], np.bincount(got["flag"].ravel(), minlength=4))
    check_unfitted_cells(mx, got, operands)
    err = fr.limit_errors(got, rld, flags == 1, tail)
    bound = 16 * max(eps, 2.0 ** -48)
    text = f"{label}: flags {np.bincount(flags.ravel(), minlength=4)}, eps {eps:.3g}, device " + ", ".join(f"{k} {v:.3g}" for k, v in err.items())
    if tail:
        eps_rel = fr.tail_errors(ref["r64"]["pval"], ref["r64"]["pval"], rld["pval"])
        err_rel = fr.tail_errors(got["pval"], ref["r64"]["pval"], rld["pval"])
        rows = len(fr.TAIL_ROWS)
        logs = [f"{math.log10(v):.1f}" if v > 0 else "-inf" for v in got["pval"][:rows, 0]]
        text += f", eps_rel {eps_rel:.3g}, |log pval - log p_LD| / max(1, |log p_LD|) {err_rel:.3g}, log10 pval of the six rows {logs}"
        print(text + f", bounds {bound:.3g} and {16 * max(eps_rel, 2.0 ** -48):.3g}")
        assert err_rel <= 16 * max(eps_rel, 2.0 ** -48)
        assert np.all(got["flag"][ref["r64"]["pval"] == 0] == 1)
    else:
        print(text + f", bound {bound:.3g}")
    assert max(err.values()) <= bound, err
    assert same(got, run(mx, plink, P, R, Wt, H, z_cutoff, penalty, tol, max_iter, dev=True))
    return got


def case_of(kind, *key):
    (codes, plink, Y, W, P, R, Wt, H), z_cutoff, tail = fr.limits_case(kind, *key)
    return (plink, P, R, Wt, H), z_cutoff, tail


@pytest.mark.parametrize("penalty", [0, 1])
@pytest.mark.parametrize("kind, key", [("bisect", (259, 1)), ("bisect", (1027, 1)), ("bisect", (259, 3)), ("alt", (259,)), ("alt", (1027,)), ("negative", (259,)),
                                       ("negative", (1027,)), ("zero", (67, 1)), ("zero", (259, 3))])
def test_the_branches_of_the_newton_loop(mx, kind, key, penalty):
    operands, z_cutoff, tail = case_of(kind, *key)
    ref = fr.limits_reference(kind, key, penalty)
    got = compare(mx, f"{kind} {key} penalty {penalty}", operands, z_cutoff, penalty, ref)
    if kind == "negative":
        assert np.all(got["score"][:9, 0] < 0) and np.all(got["flag"][:3, 0] == (1 if penalty else 2)) and np.all(got["flag"][3:6, 0] == 1)
        assert np.all(got["beta"][:9, 0][got["flag"][:9, 0] == 1] < 0)
    if kind == "zero":
        exact = ref["r64"]["z"] == 0
        assert np.array_equal(got["z"] == 0, exact) and np.all(got["score"][exact] == 0) and np.all(got["flag"][exact] == 1) and not np.any(got["flag"] == 0)
        assert np.all(got["beta"][exact] == 0) and np.all(got["chisq"][exact] == 0) and np.all(got["pval"][exact] == 1)
        assert np.array_equal(op.bits(got["se"][exact]), op.bits(1.0 / np.sqrt(got["var"][exact])))     # K''(0) = V where P = 1/2 and every term is exact


@pytest.mark.parametrize("penalty", [0, 1])
@pytest.mark.parametrize("indiv", fr.LIMITS_INDIV)
def test_a_first_step_that_saturates_every_exp_fails_beside_solved_items(mx, monkeypatch, indiv, penalty):
    operands, z_cutoff, _ = case_of("saturated", indiv)
    ref = fr.limits_reference("saturated", (indiv,), penalty)
    got = compare(mx, f"saturated {indiv} penalty {penalty}", operands, z_cutoff, penalty, ref)
    rows = 2 * len(fr.SAT_ZONES)
    assert np.all(got["flag"][:rows, 0] == 2) and (got["flag"][rows:, 0] == 1).sum() >= 2
    # exactly the one-step values, computed here from the entry's own score, var and z
    U, V, z = (got[k][:rows, 0] for k in ("score", "var", "z"))
    assert np.array_equal(op.bits(got["beta"][:rows, 0]), op.bits(U / V)) and np.array_equal(op.bits(got["se"][:rows, 0]), op.bits(1.0 / np.sqrt(V)))
    assert np.array_equal(op.bits(got["chisq"][:rows, 0]), op.bits(z * z))         # (pval: the normal p-value of mxa_assoc_score_spa, in compare)
    # the failed and the solved items share a batch whatever the batch: every pair of neighbouring marked SNPs in one, then two items a batch
    marked = np.flatnonzero(got["flag"][:, 0] != 0)
    assert np.any((got["flag"][marked[:-1], 0] == 2) & (got["flag"][marked[1:], 0] == 1))
    for name, value in (("MXA_ASSOC_SPA_BATCH", "2"), ("MXA_ASSOC_SPA_ITEMS", "2")):
        monkeypatch.setenv(name, value)
        assert same(got, run(mx, *operands, z_cutoff, penalty)), (name, value)
        monkeypatch.delenv(name)


@pytest.mark.parametrize("penalty", [0, 1])
@pytest.mark.parametrize("indiv", fr.LIMITS_TAIL_INDIV)
def test_the_deep_tail_of_the_likelihood_ratio_down_to_the_underflow_of_erfc(mx, indiv, penalty):
    operands, z_cutoff, tail = case_of("tail", indiv)
    ref = fr.limits_reference("tail", (indiv,), penalty)
    got = compare(mx, f"tail {indiv} penalty {penalty}", operands, z_cutoff, penalty, ref, tail=True)
    if indiv == 8195:
        assert (got["pval"][:len(fr.TAIL_ROWS), 0] == 0).sum() >= 2 and (indiv + 255) // 256 == 33


@pytest.mark.parametrize("penalty", [0, 1])
@pytest.mark.parametrize("index", [0, 1, 2])
def test_long_lists_every_batch_size_and_every_cut(mx, monkeypatch, index, penalty):
    operands, z_cutoff, _ = case_of("list", index)
    ref = fr.limits_reference("list", (index,), penalty)
    for name in ("MXA_ASSOC_SPA_ITEMS", "MXA_ASSOC_SPA_BATCH"):
        monkeypatch.delenv(name, raising=False)
    items = int((ref["flags"] != 0).sum())
    assert index or items > 1024
    first = compare(mx, f"list {fr.LIST_CASES[index]} penalty {penalty}, {items} items", operands, z_cutoff, penalty, ref)
    for knob_items, knob_rows in KNOBS:
        monkeypatch.setenv("MXA_ASSOC_SPA_ITEMS", str(knob_items))
        if knob_rows:
            monkeypatch.setenv("MXA_ASSOC_SPA_BATCH", str(knob_rows))
        for dev in (False, True):
            assert same(first, run(mx, *operands, z_cutoff, penalty, dev=dev)), (knob_items, knob_rows, dev)
        monkeypatch.delenv("MXA_ASSOC_SPA_BATCH", raising=False)
    monkeypatch.delenv("MXA_ASSOC_SPA_ITEMS")
    for batch in ("1", "8", "9", "257"):
        monkeypatch.setenv("MXA_ASSOC_SPA_BATCH", batch)
        for dev in (False, True):
            assert same(first, run(mx, *operands, z_cutoff, penalty, dev=dev)), (batch, dev)
    monkeypatch.delenv("MXA_ASSOC_SPA_BATCH")
    assert same(first, run(mx, *operands, z_cutoff, penalty))


@pytest.mark.parametrize("penalty", [0, 1])
def test_max_iter_2_4_6_fails_some_items_and_solves_others_in_one_launch(mx, penalty):
    operands, _, _ = case_of("bisect", 259, 1)
    zc, tol = fr.MAX_ITER_CUTOFF, fr.MAX_ITER_TOL
    full = run(mx, *operands, zc, penalty, tol=tol)
    assert np.array_equal(full["flag"], fr.max_iter_flags(penalty, 50)[0])
    for max_iter in fr.MAX_ITERS:
        flags, trace = fr.max_iter_flags(penalty, max_iter)
        assert (flags == 1).sum() >= 3 and (flags == 2).sum() >= 3
        for dev in (False, True):
            got = run(mx, *operands, zc, penalty, tol=tol, max_iter=max_iter, dev=dev)
            print(f"max_iter {max_iter} penalty {penalty} dev {dev}: flags {np.bincount(got['flag'].ravel(), minlength=4)}, the reference's "
                  f"{np.bincount(flags.ravel(), minlength=4)}")
            assert np.array_equal(got["flag"], flags), np.argwhere(got["flag"] != flags)[:5]
            check_unfitted_cells(mx, got, operands)
            on = flags == 1                        # what was accepted within max_iter evaluations is what the uncapped run accepts
            for key in FIT + ("score", "var", "z"):
                assert np.array_equal(op.bits(got[key][on]), op.bits(full[key][on])), key


@pytest.mark.parametrize("penalty", [0, 1])
@pytest.mark.parametrize("indiv", fr.LIMITS_INDIV)
@pytest.mark.parametrize("tol", fr.LIMITS_TOLS)
def test_a_loose_and_a_tight_tolerance_against_references_that_stop_as_early(mx, indiv, tol, penalty):
    operands, z_cutoff, _ = case_of("bisect", indiv, 1)
    ref = fr.limits_reference("bisect", (indiv, 1), penalty, tol, tol if tol > TOL else fr.TOL_LD)
    got = compare(mx, f"tol 2^{round(math.log2(tol))} indiv {indiv} penalty {penalty}", operands, z_cutoff, penalty, ref, tol=tol)
    if tol > TOL:
        plain = run(mx, *operands, z_cutoff, penalty)
        on = ref["flags"] == 1
        assert np.any(got["beta"][on] != plain["beta"][on]) and all(np.array_equal(op.bits(got[k][~on]), op.bits(plain[k][~on])) for k in FIT)
