"""mxa_assoc_set on the device, against the two evaluations of tests/_assoc_set_ref.py (the header's definition in np.longdouble and in plain float64 numpy).

Accuracy: for Phi and each of the six statistics the scaled error (tests/_assoc_set_ref.py: the difference over the sum of the absolute values of the terms,
taken down to the individuals) must not exceed 16 max(eps, 2^-48), eps = the same scaled error of the float64 evaluation against the long-double one on that
case.  Every figure is printed before it is asserted; the measured maxima are in DESIGN.md 3.6i.
Measured on an MI355X (the bound is 5.7e-14 in every case, eps at most 4.2e-16): Phi 9.8e-16, B 2.0e-16, varB 4.2e-16, Q 8.0e-17, c1 1.1e-15, c2 2.6e-16, c4 2.3e-16.

Shapes: the Gram tile edge is T = 16 and the split unit 4096 individuals.  indiv in {1, 5, 255, 257, 1023, 2051, 4099} (field, byte, word and wave edges; 4099
crosses the split unit: two pieces); set sizes {0, 1, 2, 15, 16, 17, 33} in every case -- an empty set, the last SNP row alone, a SNP repeated, unsorted
non-contiguous indices, a contiguous run, overlapping draws with repeats -- and one set of 1024 entries drawn from 64 SNPs at indiv = 257; (n, kh) over
{1, 2, 3} x {0, 1, 4}; missing calls at 0 and 5 %; weights NULL and random; the padding fields of every row's last byte are dirty throughout.
The raw call, the comparison on bytes, the accuracy rule and the cached cases are in tests/_assoc_set_call.py, shared with tests/test_assoc_set_limits_gpu.py."""
import numpy as np
import pytest

import _assoc_set_ref as sr
from _assoc_set_call import LD, NAMES, SNPS, _dev, call, case, check_accuracy, references, same, same_results  # noqa: F401

pytestmark = pytest.mark.gpu

#        indiv  n kh missing weights
CASES = [(1, 1, 0, 0.0, False), (5, 2, 1, 0.0, True), (255, 3, 4, 0.05, True), (257, 1, 1, 0.05, False), (1023, 2, 4, 0.0, True), (2051, 3, 0, 0.05, False),
         (4099, 1, 4, 0.05, True), (257, 2, 0, 0.05, True), (255, 3, 1, 0.0, False)]


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


@pytest.mark.parametrize("indiv,n,kh,missing,weighted", CASES)
def test_phi_and_the_statistics_against_the_long_double_reference(mx, indiv, n, kh, missing, weighted):
    codes, X, R, Wt, H, sets, weights = case(indiv, n, kh, missing, weighted)
    got = call(mx, X, indiv, R, Wt, H, sets, weights)
    eps_phi = check_accuracy(got, references(indiv, n, kh, missing, weighted), f"indiv {indiv} n {n} kh {kh}")["Phi"][1]
    # the relations: Phi exactly symmetric; its diagonal is the scan's var to the bound; the scan's own results are mxa_assoc_score's bit for bit; stat is the
    # same without the phi output and without the scan's outputs
    ld = references(indiv, n, kh, missing, weighted)[0]
    for k, s in enumerate(sets):
        for c in range(n):
            P = got["phi"][k][c]
            assert same(P, P.T.copy())
            for j, snp in enumerate(s):
                scale = float(ld[k]["sphi"][c][j, j])
                assert abs(P[j, j] - got["var"][snp, c]) <= 16 * max(eps_phi, sr.TOL) * scale, (k, c, j)
    plain = mx.assoc_score(X, SNPS, indiv, np.asfortranarray(R), np.asfortranarray(Wt), np.asfortranarray(H) if kh else None)
    for key, ref in (("score", plain.score), ("var", plain.var), ("z", plain.z), ("nobs", plain.nobs)):
        assert same(np.ascontiguousarray(got[key]), np.ascontiguousarray(np.asarray(ref).reshape(got[key].shape))), key
    bare = call(mx, X, indiv, R, Wt, H, sets, weights, scan=False, phi=False)
    assert same(bare["stat"], got["stat"])
    assert np.array_equal(got["stat"][0], np.zeros((n, 6)))                     # the empty set: sums over nothing


def test_one_set_of_1024_entries_drawn_from_64_snps(mx):
    indiv, snps, n, kh = 257, 64, 1, 1
    codes, R, Wt, H = sr.random_case(indiv, snps, n, kh, seed=9, missing=0.05)
    rng = np.random.default_rng(77)
    sets = [np.concatenate([rng.permutation(snps), rng.integers(0, snps, 1024 - snps)])]
    weights = [rng.uniform(0.3, 4.0, 1024)]
    got = call(mx, sr.pack_dirty(codes, 3), indiv, R, Wt, H, sets, weights)
    refs = (sr.set_reference(codes, R, Wt, H, sets, weights, LD), sr.set_reference(codes, R, Wt, H, sets, weights, np.float64))
    check_accuracy(got, refs, "m 1024")
    assert same(got["phi"][0][0], got["phi"][0][0].T.copy())


def test_a_single_snp_with_unit_weight_is_the_scans_own_statistic(mx):
    codes, X, R, Wt, H, _, _ = case(257, 1, 1, 0.05, False)
    got = call(mx, X, 257, R, Wt, H, [np.array([SNPS - 1])], None)                # nsets = 1, the last SNP row
    B, vB, Q, c1, c2, c4 = got["stat"][0, 0]
    U = got["score"][SNPS - 1, 0]
    P00 = got["phi"][0][0, 0, 0]
    assert B == U and Q == U * U and c1 == P00 and vB == P00 and c2 == P00 * P00 and c4 == (P00 * P00) * (P00 * P00)


def test_results_are_identical_for_every_way_of_running_the_call(mx):
    indiv, n, kh = 4099, 1, 4
    codes, X, R, Wt, H, sets, weights = case(indiv, n, kh, 0.05, True)
    base = call(mx, X, indiv, R, Wt, H, sets, weights)
    assert same_results(base, call(mx, X, indiv, R, Wt, H, sets, weights)), "two calls"
    dev = call(mx, X, indiv, R, Wt, H, sets, weights, device=True)
    assert same_results(base, dev) and all(same(np.ascontiguousarray(base[k]), np.ascontiguousarray(dev[k])) for k in ("score", "var", "z")), "device operands"
    for rows in (1, 7):
        assert same_results(base, call(mx, X, indiv, R, Wt, H, sets, weights, env=dict(MXA_ASSOC_CHUNK_ROWS=rows))), rows
    sizes = [len(s) for s in sets]
    between = sum(sizes[:4])                                                   # the list is cut behind the fourth set (and again behind every later one)
    for batch in (1, between, 10 ** 9):
        assert same_results(base, call(mx, X, indiv, R, Wt, H, sets, weights, env=dict(MXA_ASSOC_SET_BATCH=batch))), batch
        assert same_results(dev, call(mx, X, indiv, R, Wt, H, sets, weights, device=True, env=dict(MXA_ASSOC_SET_BATCH=batch))), batch
    order = [6, 2, 0, 5, 1, 4, 3]
    perm = call(mx, X, indiv, R, Wt, H, [sets[k] for k in order], [weights[k] for k in order])
    for at, k in enumerate(order):
        assert same(perm["stat"][at], base["stat"][k]) and same(perm["phi"][at], base["phi"][k]), ("permuted", k)
    keep = [1, 5, 6]
    part = call(mx, X, indiv, R, Wt, H, [sets[k] for k in keep], [weights[k] for k in keep], env=dict(MXA_ASSOC_SET_BATCH=20))
    for at, k in enumerate(keep):
        assert same(part["stat"][at], base["stat"][k]) and same(part["phi"][at], base["phi"][k]), ("subset", k)


def test_permuted_sets_subsets_and_batch_cuts_with_two_traits(mx):
    """n = 2: the blocks and the tile slots of the two traits of a set interleave in a batch; sets of 17 and 33 entries span two and three tiles"""
    indiv, n, kh = 257, 2, 0
    codes, X, R, Wt, H, sets, weights = case(indiv, n, kh, 0.05, True)
    base = call(mx, X, indiv, R, Wt, H, sets, weights)
    sizes = [len(s) for s in sets]
    for batch in (1, sum(sizes[:4]), sizes[5] + sizes[6] - 1):                 # every set alone; a cut behind the fourth set; the two largest never together
        assert same_results(base, call(mx, X, indiv, R, Wt, H, sets, weights, env=dict(MXA_ASSOC_SET_BATCH=batch))), batch
    assert same_results(base, call(mx, X, indiv, R, Wt, H, sets, weights, device=True, env=dict(MXA_ASSOC_SET_BATCH=sizes[6]))), "device operands"
    order = [5, 6, 3, 0, 2, 4, 1]
    perm = call(mx, X, indiv, R, Wt, H, [sets[k] for k in order], [weights[k] for k in order], env=dict(MXA_ASSOC_SET_BATCH=40))
    for at, k in enumerate(order):
        assert same(perm["stat"][at], base["stat"][k]) and same(perm["phi"][at], base["phi"][k]), ("permuted", k)
    keep = [6, 4]
    part = call(mx, X, indiv, R, Wt, H, [sets[k] for k in keep], [weights[k] for k in keep])
    for at, k in enumerate(keep):
        assert same(part["stat"][at], base["stat"][k]) and same(part["phi"][at], base["phi"][k]), ("subset", k)


def test_mixed_host_and_device_results_are_an_argument_error(mx):
    """score, var, zstat, stat and phi on different sides: return 1, error 1, a message that names the rule, nothing written on either side"""
    import torch
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    indiv, n, kh = 257, 1, 1
    codes, X, R, Wt, H, _, _ = case(indiv, n, kh, 0.05, False)
    sets = [np.array([1, 2, 3]), np.array([SNPS - 1])]
    ptr, idx = np.array([0, 3, 4], np.int64), np.concatenate(sets).astype(np.int32)
    ops = [np.ascontiguousarray(X), np.ascontiguousarray(R.T), np.ascontiguousarray(Wt.T), np.ascontiguousarray(H.T)]
    shapes = dict(score=(n, SNPS), var=(n, SNPS), z=(n, SNPS), stat=(6 * n, 2), phi=(10 * n,))
    sides = (dict(stat="dev", phi="host"), dict(stat="dev", score="host"), dict(stat="host", phi="dev"), dict(stat="host", score="dev"), dict(stat="host", z="dev", var="host"),
             dict(stat="dev", phi="dev", var="host"))
    for side in sides:
        outs = {k: (None if k not in side else np.full(shapes[k], -7.5) if side[k] == "host" else _dev(np.full(shapes[k], -7.5))) for k in shapes}
        nobs = np.full(SNPS, -3, np.int32)
        rc = L.mxa_assoc_set(p(ops[0]), SNPS, indiv, p(ops[1]), indiv, p(ops[2]), indiv, p(ops[3]), indiv, n, kh, 2, p(ptr), p(idx), None, p(outs["score"]), p(outs["var"]),
                             p(outs["z"]), SNPS, p(nobs), p(outs["stat"]), 2, p(outs["phi"]))
        code, text = mx.lib.last_error()
        assert (rc, code) == (1, 1) and "mxa_assoc_set" in text and "all host or all device" in text, (side, rc, code, text)
        torch.cuda.synchronize()
        for k, o in outs.items():
            if o is not None:
                assert bool((o == -7.5).all()), (side, k)
        assert np.all(nobs == -3)
    # all on the device, and all on the host, are no error
    for device in (True, False):
        call(mx, X, indiv, R, Wt, H, sets, None, device=device)


def test_an_all_missing_snp_spoils_exactly_the_sets_that_hold_it(mx):
    indiv, n, kh = 257, 2, 1
    codes, R, Wt, H = sr.random_case(indiv, SNPS, n, kh, seed=12, missing=0.05)
    codes = codes.copy()
    codes[5] = -1
    X = sr.pack_dirty(codes, 2)
    sets = [np.array([1, 2, 3]), np.array([4, 5, 6]), np.arange(6, 24), np.array([5]), np.array([0, 23, 5, 5, 9]), np.zeros(0, np.int64), np.arange(0, 5)]
    got = call(mx, X, indiv, R, Wt, H, sets, None)
    clean = [k for k, s in enumerate(sets) if 5 not in s]
    for k, s in enumerate(sets):
        finite = bool(np.all(np.isfinite(got["stat"][k])))
        assert finite == (k in clean), (k, got["stat"][k])
        if k not in clean:
            assert not np.any(np.isfinite(got["stat"][k])), (k, got["stat"][k])
    without = call(mx, X, indiv, R, Wt, H, [sets[k] for k in clean], None)
    for at, k in enumerate(clean):
        assert same(without["stat"][at], got["stat"][k]) and same(without["phi"][at], got["phi"][k]), k


@pytest.mark.parametrize("binary", [False, True])
def test_calibration_under_the_null(mx, binary):
    """indiv = 1500, 400 sets of 8 SNPs, MAF uniform in 0.01-0.05, 2 % missing calls, two covariates, omega = 1 / sqrt(f (1 - f)), seed 1: the share of sets with
    p < 0.05 must lie in [0.01, 0.09] (+-3.7 binomial standard deviations of 0.0109), for the burden and for the SKAT p-values"""
    codes, R, Wt, H, sets, weights = sr.simulate(1, binary=binary)
    res = mx.assoc_set(sr.pack(codes), codes.shape[0], codes.shape[1], R, Wt, H, sets, weights)
    for name, pv in (("burden", res.burden_p), ("skat", res.skat_p)):
        assert pv.shape == (400, 1) and np.all((pv >= 0) & (pv <= 1))
        share = float((pv < 0.05).mean())
        print("binary" if binary else "gaussian", name, "share of p < 0.05:", share)
        assert 0.01 <= share <= 0.09, (name, share)


def test_the_python_wrappers(mx):
    codes, X, R, Wt, H, sets, weights = case(255, 3, 4, 0.05, True)
    raw = call(mx, X, 255, R, Wt, H, sets, weights)
    out = dict(score=np.zeros((SNPS, 3), order="F"), nobs=np.zeros(SNPS, np.int32))
    res = mx.assoc_set(X, SNPS, 255, np.asfortranarray(R), np.asfortranarray(Wt), np.asfortranarray(H), sets, weights, out=out, want_phi=True)
    for t, field in enumerate(("burden", "burden_var", "skat", "c1", "c2", "c4")):
        assert same(np.ascontiguousarray(getattr(res, field)), np.ascontiguousarray(raw["stat"][:, :, t])), field
    assert all(same(np.ascontiguousarray(a), b) for a, b in zip(res.phi, raw["phi"]))
    assert same(np.ascontiguousarray(out["score"]), np.ascontiguousarray(raw["score"])) and same(out["nobs"], raw["nobs"])
    ptr = np.zeros(len(sets) + 1, np.int64)
    ptr[1:] = np.cumsum([len(s) for s in sets])
    csr = mx.assoc_set(X, SNPS, 255, np.asfortranarray(R), np.asfortranarray(Wt), np.asfortranarray(H), (ptr, np.concatenate(sets).astype(np.int32)), np.concatenate(weights))
    assert same(csr.skat, res.skat) and same(csr.burden, res.burden) and csr.phi is None
    live = res.c2 > 0
    assert np.all(np.isnan(res.skat_p[~live])) and np.all((res.skat_p[live] > 0) & (res.skat_p[live] <= 1)) and np.all(res.skat_df[live] <= 33 * (1 + 1e-9))
    # end to end: two 0 / 1 traits, nulls fitted on the host
    from _assoc_score_ref import binary_case
    codes, Y, W = binary_case(259, 30, 2, 2, seed=4)
    gene = [np.arange(0, 10), np.arange(10, 30), np.array([3, 29])]
    fit = mx.assoc_logistic_sets(sr.pack(codes), 30, 259, Y, W, gene)
    assert fit.skat.shape == (3, 2) and np.all(np.isfinite(fit.burden)) and np.all((fit.skat_p > 0) & (fit.skat_p <= 1)) and np.all((fit.burden_p > 0) & (fit.burden_p <= 1))
    one = mx.assoc_logistic_sets(sr.pack(codes), 30, 259, Y[:, 0], W, gene)
    assert one.skat.shape == (3,) and np.allclose(one.skat, fit.skat[:, 0], rtol=1e-10, atol=0)      # (not bit for bit: another column count of the scan)
