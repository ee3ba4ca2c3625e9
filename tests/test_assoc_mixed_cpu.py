"""miraculix_amd.mixed without a device: every argument error is a ValueError raised before the library is touched, the dense reference of the GPU tests
agrees with itself (P C = 0, gamma = 1 at h2 = 0, randomized Haseman-Elston with Hadamard probes = the exact traces), the names are re-exported, and the
library's dynamic symbol table is still exactly what the header declares: the module adds no C symbol."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

import _assoc_mixed_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNPS, INDIV = 24, 13


@pytest.fixture()
def mx(monkeypatch):
    """the package with a loader that fails when it is touched"""
    import miraculix_amd as m

    def touched(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(m.lib, "check_library_handle", touched)
    monkeypatch.setattr(m.lib, "load_shared_library", touched)
    monkeypatch.setattr(m.lib, "_LIBRARY_HANDLE", [None])
    return m


def _good():
    rng = np.random.default_rng(3)
    return dict(plink=np.zeros((SNPS, (INDIV + 3) // 4), np.uint8), snps=SNPS, indiv=INDIV, Y=rng.standard_normal((INDIV, 2)),
                covariates=rng.standard_normal((INDIV, 2)), chrom_bounds=[0, 8, 16, SNPS])


W_DEP = np.column_stack([np.arange(INDIV, dtype=np.float64), 2.0 * np.arange(INDIV) + 3.0])
SCAN_ERRORS = [
    (dict(plink=np.zeros((SNPS, 5), np.uint8)), "Matrix has wrong dimensions"),
    (dict(snps=SNPS + 1), "Matrix has wrong dimensions"),
    (dict(snps=0), "snps and indiv need to be positive"),
    (dict(Y=np.zeros((INDIV + 1, 2))), "Y needs to be"),
    (dict(Y=np.zeros((INDIV, 0))), "Y needs to be"),
    (dict(Y=np.full((INDIV, 1), np.nan)), "Y needs to be finite"),
    (dict(Y=np.full((INDIV,), np.inf)), "Y needs to be finite"),
    (dict(covariates=np.zeros((INDIV - 1, 2))), "covariates need to be"),
    (dict(covariates=np.full((INDIV, 1), np.inf)), "covariates need to be finite"),
    (dict(covariates=np.full((INDIV, 1), 2.5)), "covariate 0 is constant or depends"),
    (dict(covariates=W_DEP), "covariate 1 is constant or depends"),
    (dict(covariates=np.random.default_rng(1).standard_normal((INDIV, INDIV - 2))), "indiv needs to exceed q + 2"),
    (dict(chrom_bounds=[0, 16, 8, SNPS]), "ascending"),
    (dict(chrom_bounds=[0, 8, 8, SNPS]), "ascending"),
    (dict(chrom_bounds=[0, 6, SNPS]), "multiples of 4"),
    (dict(chrom_bounds=[0, 8, 16]), "end at snps"),
    (dict(chrom_bounds=[4, 8, SNPS]), "start at 0"),
    (dict(h2=1.0), "h2 needs to lie in [0, 1)"),
    (dict(h2=-0.1), "h2 needs to lie in [0, 1)"),
    (dict(h2=[0.2, np.nan]), "h2 needs to lie in [0, 1)"),
    (dict(h2=[0.1, 0.2, 0.3]), "one value per trait"),
    (dict(probes=0), "probes needs to be at least 1"),
    (dict(calib_snps=0), "calib_snps needs to be at least 1"),
    (dict(exact_cutoff=-1.0), "exact_cutoff must not be negative or NaN"),
    (dict(exact_cutoff=float("nan")), "exact_cutoff must not be negative or NaN"),
    (dict(tol=0.0), "tol needs to lie in (0, 1)"),
    (dict(max_iter=0), "max_iter needs to be at least 1"),
]


@pytest.mark.parametrize("bad,words", SCAN_ERRORS, ids=[f"{i}-{'-'.join(b)}" for i, (b, _) in enumerate(SCAN_ERRORS)])
def test_assoc_mixed_argument_errors_come_before_the_library(mx, bad, words):
    with pytest.raises(ValueError) as e:
        mx.assoc_mixed(**dict(_good(), **bad))
    assert words in str(e.value)


def test_the_other_entries_check_their_arguments_before_the_library(mx):
    good = _good()
    kin = types.SimpleNamespace(indiv=INDIV, nblocks=3)
    for bad, words in (dict(Y=np.zeros((INDIV + 1,))), "Y needs to be"), (dict(Y=np.full((INDIV,), np.nan)), "finite"), (dict(h2=1.5), "[0, 1)"), (dict(probes=0), "probes"), \
            (dict(covariates=np.ones((INDIV, 1))), "constant or depends"), (dict(tol=2.0), "tol"), (dict(covariates=np.zeros((INDIV, INDIV))), "q + 2"):
        with pytest.raises(ValueError) as e:
            mx.assoc_mixed_null(**dict(dict(kin=kin, Y=good["Y"], covariates=good["covariates"]), **bad))
        assert words in str(e.value)
    for bad, words in (dict(chrom_bounds=[0, 6, SNPS]), "multiples of 4"), (dict(snps=SNPS - 1), "wrong dimensions"), (dict(freq=np.zeros(SNPS + 1)), "freq needs"), \
            (dict(plink=np.zeros((SNPS, 4), np.int8)), "uint8"):
        with pytest.raises(ValueError) as e:
            mx.mixed.Kinship(**dict(dict(plink=good["plink"], snps=SNPS, indiv=INDIV, chrom_bounds=good["chrom_bounds"]), **bad))
        assert words in str(e.value)
    for bad, words in (dict(tol=0.0), "tol needs"), (dict(max_iter=0), "max_iter needs"), (dict(tau=-1.0), "tau must not"), (dict(tau=float("nan")), "tau must not"), \
            (dict(), "B needs to be a float64"):                                  # a host B is refused last: the solver works on device tensors only
        with pytest.raises(ValueError) as e:
            mx.mixed.solve(**dict(dict(kin=kin, tau=1.0, B=np.zeros((INDIV, 1)), tol=1e-10, max_iter=5), **bad))
        assert words in str(e.value)


def test_the_names_are_re_exported_and_the_basis_matches_the_reference(mx):
    assert mx.assoc_mixed is mx.mixed.assoc_mixed and mx.assoc_mixed_null is mx.mixed.assoc_mixed_null
    assert mx.mixed.MixedNull._fields == ("h2", "tau", "gamma", "r", "sigma2", "VinvC", "G_chol", "Qc", "iters")
    assert mx.mixed.AssocMixedResult._fields == ("score", "var", "zstat", "pval", "beta", "se", "flag", "h2", "gamma", "nobs")
    C = np.column_stack([np.ones(INDIV), _good()["covariates"]])
    Q = mx.mixed.gram_schmidt_twice(C)
    assert np.array_equal(Q, mr.gram_schmidt_twice(C)) and np.abs(Q.T @ Q - np.eye(3)).max() <= 8 * 2.0 ** -52
    # the seeded draws: the library's recipe and the reference's give the same probes and picks
    assert np.array_equal(mx.mixed.rademacher(INDIV, 5, 9).numpy(), mr.rademacher(INDIV, 5, 9)) and set(np.unique(mr.rademacher(INDIV, 5, 9))) == {-1.0, 1.0}
    assert np.array_equal(mx.mixed.calibration_picks(40, 7, 3, 2), mr.picks(40, 7, 3, 2)) and mr.picks(5, 9, 1, 0).tolist() == [0, 1, 2, 3, 4]


def test_the_module_adds_no_symbol_to_the_library():
    """the dynamic symbol table is what the header declares (the pattern of tests/test_abi_cpu.py), and the module names no entry the header does not have"""
    header = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "miraculix_amd.h")).read(), flags=re.S), flags=re.M)
    declared = set(re.findall(r"\b(\w+)\s*\([^;{]*\)\s*;", header))
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "miraculix_amd", "lib", "libmiraculix_amd.so")],
                                                                 text=True).splitlines() if ln.strip()}
    assert exported == declared, exported ^ declared
    assert not [s for s in declared if "mixed" in s]
    source = open(os.path.join(ROOT, "miraculix_amd", "mixed.py")).read()
    assert set(re.findall(r"\bmxa_\w+", source)) <= declared


# ---------------------------------------------------------------------------------------------------------- the reference against itself
@pytest.fixture(scope="module")
def dense_case():
    indiv, snps, bounds = 64, 240, [0, 80, 160, 240]
    codes = mr.random_codes(snps, indiv, seed=5, missing=0.03)
    rng = np.random.default_rng(6)
    W = rng.standard_normal((indiv, 2)) + 1.5
    Y = rng.standard_normal((indiv, 2)) + W @ rng.standard_normal((2, 2))
    return codes, bounds, Y, W


def test_pack_and_unpack_are_inverse(dense_case):
    codes = dense_case[0]
    assert np.array_equal(mr.unpack(mr.pack(codes), codes.shape[1]), codes)
    assert np.array_equal(mr.unpack(mr.pack(codes[:, :61]), 61), codes[:, :61])


def test_the_projection_annihilates_the_covariates(dense_case):
    codes, bounds, Y, W = dense_case
    C, _ = mr.design(codes.shape[1], W)
    for leave in (None, 1):
        K = mr.kinship_dense(codes, bounds, leave)
        assert np.array_equal(K, K.T) or np.abs(K - K.T).max() <= 2.0 ** -50 * np.abs(K).max()
        for nr in mr.null_ref(K, Y, C, np.array([0.3, 0.7])):
            scale = np.abs(nr["P"]).max() * np.abs(C).max()
            assert np.abs(nr["P"] @ C).max() <= 1e-10 * scale                      # rounding of a solve with cond(G) ~ 1e2 and 64 terms
            assert abs(nr["r"] @ C).max() <= 1e-10 * np.abs(nr["r"]).max() * np.abs(C).max()


def test_the_calibration_factor_is_one_without_heritability(dense_case):
    codes, bounds, Y, W = dense_case
    for loco in (True, False):
        res = mr.mixed_ref(codes, bounds, Y, W, loco=loco, h2=0.0, calib_snps=50)
        assert res["gamma"].shape == ((3, 2) if loco else (1, 2))
        assert np.abs(res["gamma"] - 1.0).max() <= 1e-12
        # and the scan is then the plain score test
        ols = mr.ols_ref(codes, Y, W)
        assert np.nanmax(np.abs(res["z"] - ols)) <= 1e-10 * np.nanmax(np.abs(ols))


def test_randomized_haseman_elston_with_hadamard_probes_is_exact(dense_case):
    codes, bounds, Y, W = dense_case
    indiv = codes.shape[1]
    _, Qc = mr.design(indiv, W)
    K = mr.kinship_dense(codes, bounds)
    H = mr.hadamard(indiv)
    assert np.array_equal(H @ H.T, indiv * np.eye(indiv))
    M = np.eye(indiv) - Qc @ Qc.T
    Kt = M @ K @ M
    # unclipped: compare the estimating equations' solution itself
    t1, t2 = np.mean(np.sum(H * (Kt @ H), 0)), np.mean(np.sum((Kt @ H) ** 2, 0))
    assert abs(t1 - np.trace(Kt)) <= 1e-12 * abs(np.trace(Kt)) and abs(t2 - np.sum(Kt * Kt)) <= 1e-12 * np.sum(Kt * Kt)
    assert np.abs(mr.he_estimate(K, Y, Qc, H) - mr.he_exact(K, Y, Qc)).max() <= 1e-11


def test_the_block_cg_reference_solves_and_freezes(dense_case):
    codes, bounds, _, _ = dense_case
    indiv = codes.shape[1]
    A = 2.0 * mr.kinship_dense(codes, bounds) + np.eye(indiv)
    B = np.random.default_rng(2).standard_normal((indiv, 4))
    B[:, 2] = 0.0
    X, iters, relres = mr.block_cg(A, B)
    ref = np.linalg.solve(A, B)
    assert iters[2] == 0 and np.all(iters[[0, 1, 3]] > 0) and np.all(relres <= 1e-10) and np.array_equal(X[:, 2], np.zeros(indiv))
    assert np.abs(X - ref).max() <= np.linalg.cond(A) * 1e-10 * np.abs(ref).max()


def test_the_structured_case_is_what_the_inflation_test_needs():
    """the data of the GPU inflation test, chosen here with the dense reference alone (seed 2, shift 0.4, h2g 0.3): plain OLS lambda_GC 2.156, mixed 0.977"""
    codes, y, pop = mr.structured_case(401, 1200, seed=2, shift=0.4, h2g=0.3)
    assert codes.shape == (1200, 401) and codes.min() == 0 and codes.max() == 2 and pop.sum() in (200, 201)
    ols = mr.lambda_gc(mr.ols_ref(codes, y))
    mixed = mr.lambda_gc(mr.mixed_ref(codes, [0, 400, 800, 1200], y)["z"])
    print("lambda_GC: OLS", ols, "mixed", mixed)
    assert ols > 1.5 and 0.85 <= mixed <= 1.15
    assert abs(ols - 2.156) <= 2e-3 and abs(mixed - 0.977) <= 2e-3
