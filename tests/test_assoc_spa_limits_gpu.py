"""mxa_assoc_score_spa where its lists, batches and tails had never run (tests/test_assoc_spa_gpu.py stops at 130 SNPs, some 20 marked SNPs, 19 columns of B,
max_iter in {1, 50}, tol 2^-30 and p > 1e-200).  The cases and their references are built in tests/_assoc_spa_ref.py; tests/test_assoc_spa_limits_cpu.py
asserts the conditions on the inputs without a device.  The comparison is that module's: flags equal to both references' everywhere; score, var, z and nobs
bit for bit mxa_assoc_score's; |log pval - log p_LD| <= 16 max(eps, 2^-48), eps = the case's largest |log p_64 - log p_LD|; host and device operands, and
every batch size, give the same bits.

What each test reaches in mxa_assoc_spa.hip that the suite had not:
  many_marked_snps    k_assoc_spa_list: rounds beyond the first of `for (s0 ...; s0 += 256)` with base_k and base_item carried, both spa_block_scan calls on
                      the same LDS array per round, a partial last round.  k_assoc_spa_items and k_assoc_spa_combine: blockIdx.x > 0 (577 and 269 marked SNPs,
                      1145 and 716 items).  k_assoc_spa_form with n = 8, and with n (kh + 2) = 36: a_j read from the columns 6 ... 35 of D and M, the last four of
                      them in the product's second chunk of 32 columns.
  round_boundaries    the same loop with marks at the first and last thread of a round, a round without a mark (tot_k = 0), a round entirely marked, a last
                      round of 6 SNPs; entirely missing rows between them.  spa_stage's gather for a host matrix (assoc_gather_rows): one run of 1030 rows, and 515 single
                      rows.
                      MXA_ASSOC_SPA_BATCH in {1, 8, 9, 257}: batches that end on, before and after a tile of kSpaTile = 8, and one past 256 marked SNPs.
  item_cut            spa_stage: `off[k1 + 1] - off[k0] <= max_items` ends batches (MXA_ASSOC_SPA_ITEMS), alone, with the row cut, and raised to n ("one SNP's
                      items always fit"); k_assoc_spa_form with item_base = off[k0] > 0 and tiles counted from a k0 that is no multiple of 8.
  max_iter            k_assoc_spa, in spa_newton_step: `evals >= max_iter` behind the bracket check on some sides while others of the same batch are accepted; k_assoc_spa_combine:
                      `b.status == kSpaFailed` and `a.status != kSpaSolved` beside solved items.
  loose_tol           k_assoc_spa, in spa_newton_step: `fabs(tn - t) <= tol * fabs(tn)` with a tol that ends the loop an evaluation earlier than 2^-30.
  deep_tail           k_assoc_spa: the tail 0.5 erfc(zeta / sqrt 2) from 1e-14 down to 7e-290 and past the underflow of erfc.

Measured on an MI355X (flags as [0, 1, 2, 3]; eps seen on x86-64 with 80-bit long double / the device's largest |log pval - log p_LD|):
  (67, 700, 3, 1, z 0.5)    577 marked SNPs, 1145 items, flags [955, 1145, 0, 0]: 2.5e-14 / 2.3e-14
  (259, 300, 8, 2, z 1)     269 marked SNPs, 716 items, flags [1684, 716, 0, 0]: 1.3e-14 / 2.6e-14
  (259, 33, 3, 10, z 1)     21 marked SNPs, 30 items, flags [69, 30, 0, 0]: 1.9e-15 / 3.4e-15
  layouts of (67, 130, 2, 1, z 1.5), 1030 SNPs each, eps 2.0e-14: edges 6 marked SNPs, 9 items, flags [2047, 9, 0, 4]: 3.2e-15; empty_and_full 257 and 386,
                            [1674, 386, 0, 0]: 6.9e-15; all_loud 1030 and 1545, [515, 1545, 0, 0]: 6.9e-15; alternating 515 and 773, [1287, 773, 0, 0]: 6.9e-15
  max_iter on (259, 300, 8, 2, z 1)    flags [1684, 7, 709, 0] (max_iter 4), [1684, 609, 107, 0] (6), [1684, 705, 11, 0] (8): the references' own
  tol 2^-12 on (259, 130, 3, 3, z 2)   flags [367, 23, 0, 0]: 5.9e-15 / 3.4e-15
  the tail (eps_rel / the device's largest |log pval - log p_LD| / max(1, |log p_LD|); log10 pval of the six rows):
    1027 (45 cases)     flags [10, 14, 0, 0]: 2.2e-14 / 1.4e-14; -66.9, -62.5, -30.5, -14.1, -59.3, -48.3
    4099 (180 cases)    flags [12, 12, 0, 0]: 6.0e-14 / 6.9e-14; -289.2, -269.7, -126.4, -60.1, -253.5, -202.4
    8195 (350 cases)    flags [15, 9, 0, 0]: 6.4e-14 / 7.5e-14; 0, 0, -249.5, -120.0, 0, 0 (exactly 0 with the flag 1 where erfc underflows)
  The relative bound 16 max(eps_rel, 2^-48) holds down to 7e-290: the device's erfc needs no allowance of its own.
"""
import functools
import math

import numpy as np
import pytest

import _assoc_spa_ref as sp
import _operands as op
from test_assoc_spa_gpu import MAX_ITER, TOL, log_error, run, run_score, same

pytestmark = pytest.mark.gpu

#        MXA_ASSOC_SPA_ITEMS, MXA_ASSOC_SPA_BATCH (None: unset).  On (67, 700, 3, 1) the first four are cut by the items alone, (7, 9) too (nine SNPs hold at
#        least nine items), (1000, 3) by the rows alone, and (4, 3) by the items in some batches and by the rows in others.
KNOBS = [(1, None), (4, None), (7, None), (1000, None), (7, 9), (1000, 3), (4, 3)]


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


def compare(mx, label, plink, operands, z_cutoff, pld, flags, eps, tol=TOL, max_iter=MAX_ITER):
    """the comparison rule of the module's docstring on one call with host operands, then the same call with device operands: the same bits.  Returns the
    host call's result."""
    P, R, Wt, H = operands
    got = run(mx, plink, P, R, Wt, H, z_cutoff, tol, max_iter)
    (score, var, z), nobs = run_score(mx, plink, R, Wt, H)
    for name, want in (("score", score), ("var", var), ("z", z), ("nobs", nobs)):
        assert np.array_equal(op.bits(got[name]), op.bits(want)), name
    assert np.array_equal(got["flag"], flags), np.argwhere(got["flag"] != flags)[:5]
    err, count = log_error(got["pval"], pld)
    bound = 16 * max(eps, 2.0 ** -48)
    print(f"{label}: flags {np.bincount(flags.ravel(), minlength=4)}, eps {eps:.3g}, max |log pval - log p_LD| {err:.3g} over {count} entries, bound {bound:.3g}")
    assert err <= bound
    assert same(got, run(mx, plink, P, R, Wt, H, z_cutoff, tol, max_iter, dev=True))
    return got


@pytest.mark.parametrize("indiv, snps, n, kh, z_cutoff, marked_above", [c + (m,) for c, m in zip(sp.LIST_CASES, (512, 256, 0))])
def test_many_marked_snps_list_rounds_item_blocks_and_36_columns(mx, indiv, snps, n, kh, z_cutoff, marked_above):
    codes, plink, Y, W, P, R, Wt, H = sp.limits_operands(indiv, snps, n, kh)
    ref = sp.limits_reference(indiv, snps, n, kh, z_cutoff)
    marked = int((ref["flags"] == 1).any(axis=1).sum())
    assert marked > marked_above and (marked_above or n * (kh + 2) > 32)
    compare(mx, f"indiv {indiv} snps {snps} n {n} kh {kh} z_cutoff {z_cutoff}, {marked} marked SNPs, {int((ref['flags'] == 1).sum())} items", plink, (P, R, Wt, H),
            z_cutoff, ref["pld"], ref["flags"], ref["eps"])


@functools.lru_cache(maxsize=None)
def layout(name):
    """(packed rows, p_LD, flags, eps) of a layout of the pool: the pool's references indexed by the layout"""
    pool = sp.pool()
    rows, ref = pool["layouts"][name], pool["ref"]
    return sp.frozen(sp.pack(pool["codes"][rows]), ref["pld"][rows], ref["flags"][rows]) + (sp.log_eps(ref["p64"][rows], ref["pld"][rows]),)


@pytest.mark.parametrize("name, marked", [("edges", 6), ("empty_and_full", 257), ("all_loud", 1030), ("alternating", 515)])
def test_marks_on_the_round_boundaries_and_every_batch_size(mx, monkeypatch, name, marked):
    pool = sp.pool()
    P, R, Wt, H = pool["operands"]
    assert len(pool["two"]) >= 1 and len(pool["one"]) >= 1 and len(pool["two"]) + len(pool["one"]) >= 4 and len(pool["quiet"]) >= 4
    plink, pld, flags, eps = layout(name)
    assert plink.shape[0] == sp.ROUNDS_TOTAL and (flags == 1).any(axis=1).sum() == marked
    first = compare(mx, f"layout {name}, {marked} marked SNPs, {int((flags == 1).sum())} items", plink, pool["operands"], pool["z_cutoff"], pld, flags, eps)
    if name == "edges":
        assert np.all(np.isnan(first["pval"][[254, 768]])) and np.all(first["nobs"][[254, 768]] == 0)
    for batch in ("1", "8", "9", "257"):
        monkeypatch.setenv("MXA_ASSOC_SPA_BATCH", batch)
        for dev in (False, True):
            assert same(first, run(mx, plink, P, R, Wt, H, pool["z_cutoff"], dev=dev)), (batch, dev)
    monkeypatch.delenv("MXA_ASSOC_SPA_BATCH")


@pytest.mark.parametrize("which", ["list", "edges"])
def test_the_item_cut_alone_with_the_row_cut_and_raised_to_n(mx, monkeypatch, which):
    if which == "list":
        indiv, snps, n, kh, z_cutoff = sp.LIST_CASES[0]
        _, plink, _, _, P, R, Wt, H = sp.limits_operands(indiv, snps, n, kh)
        flags = sp.limits_reference(indiv, snps, n, kh, z_cutoff)["flags"]
    else:
        pool = sp.pool()
        (P, R, Wt, H), z_cutoff = pool["operands"], pool["z_cutoff"]
        plink, _, flags, _ = layout("edges")
    monkeypatch.delenv("MXA_ASSOC_SPA_ITEMS", raising=False)
    monkeypatch.delenv("MXA_ASSOC_SPA_BATCH", raising=False)
    first = run(mx, plink, P, R, Wt, H, z_cutoff)
    assert np.array_equal(first["flag"], flags)
    for items, rows in KNOBS:
        monkeypatch.setenv("MXA_ASSOC_SPA_ITEMS", str(items))
        if rows:
            monkeypatch.setenv("MXA_ASSOC_SPA_BATCH", str(rows))
        for dev in (False, True):
            assert same(first, run(mx, plink, P, R, Wt, H, z_cutoff, dev=dev)), (items, rows, dev)
        monkeypatch.delenv("MXA_ASSOC_SPA_BATCH", raising=False)
    monkeypatch.delenv("MXA_ASSOC_SPA_ITEMS")
    assert same(first, run(mx, plink, P, R, Wt, H, z_cutoff))


@functools.lru_cache(maxsize=None)
def long_double_evaluations_at_the_entrys_stop():
    indiv, snps, n, kh, z_cutoff = sp.MAX_ITER_CASE
    codes, _, _, _, P, R, Wt, H = sp.limits_operands(indiv, snps, n, kh)
    return sp.spa_reference(codes, P, R, Wt, H, z_cutoff, TOL, MAX_ITER, sp.LD)[3]


@pytest.mark.parametrize("max_iter", [4, 6, 8])
def test_a_max_iter_that_fails_some_sides_and_solves_others(mx, max_iter):
    indiv, snps, n, kh, z_cutoff = sp.MAX_ITER_CASE
    codes, plink, Y, W, P, R, Wt, H = sp.limits_operands(indiv, snps, n, kh)
    ref = sp.limits_reference(indiv, snps, n, kh, z_cutoff)
    # the float64 and the long-double reference need the same number of evaluations on every item at the entry's stop rule: rounding decides no flag
    assert np.array_equal(long_double_evaluations_at_the_entrys_stop(), ref["e64"])
    _, flags, _, _, _ = sp.spa_reference(codes, P, R, Wt, H, z_cutoff, TOL, max_iter, np.float64)
    assert (flags == 1).sum() >= 5 and (flags == 2).sum() >= 5
    full = run(mx, plink, P, R, Wt, H, z_cutoff)
    normal = run(mx, plink, P, R, Wt, H, math.inf)
    assert np.array_equal(full["flag"], ref["flags"]) and np.all(normal["flag"] == 0)
    for dev in (False, True):
        got = run(mx, plink, P, R, Wt, H, z_cutoff, max_iter=max_iter, dev=dev)
        print(f"max_iter {max_iter}, dev {dev}: flags {np.bincount(got['flag'].ravel(), minlength=4)}, the reference's {np.bincount(flags.ravel(), minlength=4)}")
        assert np.array_equal(got["flag"], flags), np.argwhere(got["flag"] != flags)[:5]
        failed = flags == 2
        assert np.array_equal(op.bits(got["pval"][failed]), op.bits(normal["pval"][failed]))
        assert np.array_equal(op.bits(got["pval"][~failed]), op.bits(full["pval"][~failed]))
        for key in ("score", "var", "z", "nobs"):
            assert np.array_equal(op.bits(got[key]), op.bits(full[key])), key


def test_a_loose_tolerance_against_references_that_stop_as_early(mx):
    indiv, snps, n, kh, z_cutoff = sp.LOOSE_TOL_CASE
    codes, plink, Y, W, P, R, Wt, H = sp.limits_operands(indiv, snps, n, kh)
    ref = sp.limits_reference(indiv, snps, n, kh, z_cutoff, sp.LOOSE_TOL, sp.LOOSE_TOL)
    assert np.array_equal(ref["e64"], ref["eld"])
    got = compare(mx, f"indiv {indiv} snps {snps} n {n} kh {kh} z_cutoff {z_cutoff} tol 2^-12", plink, (P, R, Wt, H), z_cutoff, ref["pld"], ref["flags"], ref["eps"],
                  tol=sp.LOOSE_TOL)
    tight = run(mx, plink, P, R, Wt, H, z_cutoff)
    on = ref["flags"] == 1
    assert np.any(got["pval"][on] != tight["pval"][on]) and np.array_equal(op.bits(got["pval"][~on]), op.bits(tight["pval"][~on]))


@pytest.mark.parametrize("indiv", sp.TAIL_INDIV)
def test_the_deep_tail_down_to_the_underflow_of_erfc(mx, indiv):
    codes, plink, Y, W, P, R, Wt, H = sp.tail_operands(indiv)
    ref = sp.tail_reference(indiv)
    rows = len(sp.TAIL_ROWS)
    assert np.all(ref["flags"][:rows] == 1) and max(ref["e64"].max(), ref["eld"].max()) <= 12
    bound = 16 * max(ref["eps_rel"], 2.0 ** -48)
    for dev in (False, True):
        got = run(mx, plink, P, R, Wt, H, 1.0, dev=dev)
        assert np.array_equal(got["flag"], ref["flags"]), np.argwhere(got["flag"] != ref["flags"])[:5]
        err = sp.tail_errors(got["pval"], ref["p64"], ref["pld"])
        logs = [f"{math.log10(v):.1f}" if v > 0 else "-inf" for v in got["pval"][:rows, 0]]
        print(f"indiv {indiv}, dev {dev}: {int(Y.sum())} cases, flags {np.bincount(ref['flags'].ravel(), minlength=4)}, log10 pval of the six rows {logs}, "
              f"eps_rel {ref['eps_rel']:.3g}, max |log pval - log p_LD| / max(1, |log p_LD|) {err:.3g}, bound {bound:.3g}")
        assert err <= bound
        zero = ref["p64"] == 0
        assert np.all(got["flag"][zero] == 1)
    assert same(got, run(mx, plink, P, R, Wt, H, 1.0))
