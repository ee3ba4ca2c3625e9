"""miraculix_amd.mixed on the device against the dense reference tests/_assoc_mixed_ref.py (K formed, np.linalg.solve).

The tolerance of everything behind a solve.  A CG residual of tol bounds the relative error of the solution by kappa tol, kappa <= 1 + tau lambda_max(K) (the
smallest eigenvalue of tau K + I is at least 1); lambda_max comes from the dense K of the test.  Asserted: |got - ref| <= F kappa tol scale, scale = the largest
absolute reference value of the array, for r, gamma (GLS and calibration), sigma2, U, V and z, with F kappa tol <= 1e-6 required of every case.
F = 8 x the largest ratio |got - ref| / (kappa tol scale) observed on an MI355X over all cases of this file (the ratios are printed before they are asserted):

    case                              r      GLS gamma  sigma2   U      V        z      calibration  beta   se       pval
    203-n1-q0-given-loco              0.143  0.0067     1e-5     0.136  3e-5     0.136  3e-5         0.175  1e-5     0.106
    256-n3-q2-estimated-loco-exact    0.440  0.019      0.033    0.341  0.074    0.337  6e-4         0.444  0.040    0.262
    401-n3-q2-given-whole-exact       0.211  0.016      0.0096   0.247  0.012    0.244  2e-4         0.237  0.0053   0.178
    401-n1-q2-estimated-whole         0.306  0.023      0.0078   0.344  0.0082   0.335  4e-4         0.203  0.0041   0.258
    single block (203, given)                                    0.094  4e-5     0.095  3e-5         0.092  1e-5     0.074
    solve (401, 4 columns, tau 1.5): X 0.072 with every block, 0.112 without block 1; 22 and 25 iterations, as the numpy recurrence takes
    host / device plink and Y: the ratios of the second case, to the digits shown
    Kinship.apply: at most 1.5e-15 max|K V| over all shapes, n and left-out blocks

The largest is 0.444 (beta of the second case; of the arrays named above: r 0.440), so F = 3.552, and F kappa tol <= 1.3e-9 with kappa <= 3.54.

Kinship.apply alone is two chained centred products: the bound 1e-11 max|K V| is the one tests/test_cg_gpu.py::test_gram_matvec_matches_two_products_and_oracle
asserts for mxa_gram_matvec against the dense oracle."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _assoc_mixed_ref as mr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10
OBSERVED = 0.444         # largest |got - ref| / (kappa tol scale) seen on the MI355X
F = 8 * OBSERVED
EVEN, RAGGED = (0, 400, 800, 1200), (0, 396, 800, 1200)


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    m.dgemm_compressed.set_options(use_gpu=True, not_center=False, verbose=0)
    return m


@functools.lru_cache(maxsize=None)
def data(indiv, n, q, missing, seed=1):
    """codes, Y (indiv, n), W (indiv, q) or None: random genotypes, a phenotype with a polygenic part from every 10th SNP"""
    codes = mr.random_codes(1200, indiv, seed, missing)
    rng = np.random.default_rng([seed, indiv, n, q])
    W = rng.standard_normal((indiv, q)) + rng.uniform(-2, 2, q) if q else None
    x, _ = mr.imputed(codes[::10])
    g = (x - x.mean(1, keepdims=True)).T @ rng.standard_normal((x.shape[0], n))
    Y = 0.7 * g / g.std(0) + rng.standard_normal((indiv, n)) + (W @ rng.standard_normal((q, n)) if q else 0.0)
    return codes, mr.pack(codes), np.asfortranarray(Y), W


def ratio(got, ref, kappa, what, mask=None):
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    got, ref = np.asarray(got, np.float64).reshape(np.shape(ref)), np.asarray(ref, np.float64)
    ok = np.isfinite(ref) if mask is None else mask
    assert np.all(np.isfinite(got[ok])), what
    val = float(np.abs(got[ok] - ref[ok]).max() / (kappa * TOL * np.abs(ref[ok]).max()))
    print(f"  ratio {what:>12s} {val:.3e}")
    return val


def test_kinship_apply_against_the_dense_matrix(mx):
    import torch
    for indiv, bounds, missing in ((203, EVEN, 0.03), (256, RAGGED, 0.0), (401, RAGGED, 0.03)):
        codes, plink, _, _ = data(indiv, 1, 0, missing)
        with mx.mixed.Kinship(plink, 1200, indiv, bounds) as kin:
            assert kin.nblocks == 3 and kin.bounds == list(bounds)
            for n in (1, 5):
                V = np.random.default_rng(n).standard_normal((indiv, n))
                Vd = torch.from_numpy(V).cuda()
                for leave in (None, 0, 2):
                    ref = mr.kinship_dense(codes, bounds, leave) @ V
                    got = kin.apply(Vd, leave).cpu().numpy()
                    err = np.abs(got - ref).max() / np.abs(ref).max()
                    print(f"apply indiv {indiv} n {n} leave_out {leave}: {err:.3e}")
                    assert err <= 1e-11
            with pytest.raises(ValueError):
                kin.apply(Vd, 3)
            with pytest.raises(ValueError):
                kin.apply(V)
        with pytest.raises(RuntimeError):
            kin.apply(Vd)


def test_solve_against_a_dense_solve(mx):
    import torch
    indiv, tau = 401, 1.5
    codes, plink, _, _ = data(indiv, 1, 0, 0.03)
    B = np.random.default_rng(4).standard_normal((indiv, 4))
    B[:, 2] = 0.0
    with mx.mixed.Kinship(torch.from_numpy(plink).cuda(), 1200, indiv, RAGGED) as kin:
        for leave in (None, 1):
            K = mr.kinship_dense(codes, RAGGED, leave)
            A = tau * K + np.eye(indiv)
            kappa = 1.0 + tau * float(np.linalg.eigvalsh(K)[-1])
            assert F * kappa * TOL <= 1e-6
            ref = np.linalg.solve(A, B)
            _, ref_iters, _ = mr.block_cg(A, B, TOL)
            Bd = torch.from_numpy(B).cuda()
            X, iters, relres = mx.mixed.solve(kin, tau, Bd, leave, tol=TOL)
            iters, relres = iters.cpu().numpy(), relres.cpu().numpy()
            print("iterations", iters, "reference", ref_iters, "relres", relres)
            assert iters[2] == 0 and relres[2] == 0 and not X[:, 2].any()
            assert np.all(relres <= TOL) and np.all(np.abs(iters - ref_iters) <= 1) and np.all(iters[[0, 1, 3]] > 1)
            assert ratio(X, ref, kappa, "X") <= F
            x1, it1, _ = mx.mixed.solve(kin, tau, Bd[:, 3:4], leave, tol=TOL)
            assert abs(int(it1[0]) - ref_iters[3]) <= 1
            assert np.abs((x1[:, 0] - X[:, 3]).cpu().numpy()).max() <= 2 * F * kappa * TOL * np.abs(ref[:, 3]).max()
        with pytest.raises(RuntimeError, match="column 0 has not converged after 2 iterations"):
            mx.mixed.solve(kin, tau, Bd, tol=TOL, max_iter=2)


CASES = {
    "203-n1-q0-given-loco": dict(indiv=203, n=1, q=0, missing=0.0, bounds=EVEN, h2=0.4, loco=True, exact=None),
    "256-n3-q2-estimated-loco-exact": dict(indiv=256, n=3, q=2, missing=0.03, bounds=EVEN, h2=None, loco=True, exact=1.0),
    "401-n3-q2-given-whole-exact": dict(indiv=401, n=3, q=2, missing=0.03, bounds=RAGGED, h2=(0.2, 0.5, 0.2), loco=False, exact=1.0),
    "401-n1-q2-estimated-whole": dict(indiv=401, n=1, q=2, missing=0.0, bounds=RAGGED, h2=None, loco=False, exact=None),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    c = CASES[name]
    codes, _, Y, W = data(c["indiv"], c["n"], c["q"], c["missing"])
    return mr.mixed_ref(codes, c["bounds"], Y, W, loco=c["loco"], h2=c["h2"], calib_snps=60, exact_cutoff=c["exact"], seed=3, probes=16)


def check_scan(res, ref, what):
    kappa = ref["kappa"]
    assert F * kappa * TOL <= 1e-6, kappa
    print(f"{what}: kappa {kappa:.2f} h2 {ref['h2']} gamma {ref['gamma'].ravel()}")
    flag = res.flag.cpu().numpy() if hasattr(res.flag, "cpu") else res.flag
    assert flag.dtype == np.int32 and np.array_equal(flag, ref["flag"])
    worst = max(ratio(res.score, ref["score"], kappa, "U"), ratio(res.var, ref["var"], kappa, "V"), ratio(res.zstat, ref["z"], kappa, "z"),
                ratio(res.gamma, ref["gamma"], kappa, "calibration"), ratio(res.beta, ref["beta"], kappa, "beta"), ratio(res.se, ref["se"], kappa, "se"))
    assert np.abs(res.h2 - ref["h2"]).max() <= F * kappa * TOL
    big = ref["pval"] > 1e-300                       # |dp| <= 0.8 |dz| <= 0.8 F kappa tol max|z|, and the largest p-value is about 1
    assert ratio(res.pval, ref["pval"], kappa * max(1.0, float(np.nanmax(np.abs(ref["z"])))), "pval", big & np.isfinite(ref["pval"])) <= F
    assert worst <= F, worst
    return worst


@pytest.mark.parametrize("name", list(CASES))
def test_null_model_and_scan_against_the_reference(mx, name):
    c, ref = CASES[name], reference(name)
    indiv, n = c["indiv"], c["n"]
    _, plink, Y, W = data(indiv, n, c["q"], c["missing"])
    kappa = ref["kappa"]
    leave = 0 if c["loco"] else None
    with mx.mixed.Kinship(plink, 1200, indiv, c["bounds"]) as kin:
        null = mx.assoc_mixed_null(kin, Y, W, h2=c["h2"], probes=16, seed=3, leave_out=None, tol=TOL)
        assert np.abs(null.h2 - ref["h2"]).max() <= F * kappa * TOL                      # the estimate on the full K, from the same probes
        null = mx.assoc_mixed_null(kin, Y, W, h2=ref["h2"], leave_out=leave, tol=TOL)
    nr = ref["nulls"][0]
    assert null.r.shape == (indiv, n) and null.gamma.shape == (c["q"] + 1, n) and null.Qc.shape == (indiv, c["q"] + 1) and np.all(null.iters >= 1)
    worst = max(ratio(null.r, np.stack([t["r"] for t in nr], 1), kappa, "r"), ratio(null.gamma, np.stack([t["gamma"] for t in nr], 1), kappa, "GLS gamma"),
                ratio(null.sigma2, np.array([t["sigma2"] for t in nr]), kappa, "sigma2"))
    assert np.array_equal(null.tau, np.array([t["tau"] for t in nr]))
    assert worst <= F, worst
    res = mx.assoc_mixed(plink, 1200, indiv, Y, W, chrom_bounds=c["bounds"], loco=c["loco"], h2=c["h2"], calib_snps=60, exact_cutoff=c["exact"], seed=3, probes=16, tol=TOL)
    assert isinstance(res.score, np.ndarray) and res.score.shape == (1200, n) and res.gamma.shape == ((3 if c["loco"] else 1), n)
    codes = data(indiv, n, c["q"], c["missing"])[0]
    assert res.nobs.dtype == np.int32 and np.array_equal(res.nobs, (codes >= 0).sum(1))
    if c["exact"] is not None:
        share = ref["flag"].mean()
        print("share of the exact stage", share)
        assert 0.2 <= share <= 0.5                                                       # |z| >= 1 under the null: about 0.32
    else:
        assert not ref["flag"].any()
    check_scan(res, ref, name)


def test_loco_with_a_single_block_falls_back(mx):
    indiv = 203
    codes, plink, Y, _ = data(indiv, 1, 0, 0.0)
    ref = mr.mixed_ref(codes, (0, 1200), Y, None, loco=True, h2=0.4, calib_snps=60, seed=3)
    res = mx.assoc_mixed(plink, 1200, indiv, Y, loco=True, h2=0.4, calib_snps=60, seed=3, tol=TOL)
    assert res.gamma.shape == (1, 1) and ref["gamma"].shape == (1, 1)
    check_scan(res, ref, "single block")


def test_the_mixed_model_removes_the_inflation_the_linear_scan_has(mx):
    """The reason for the feature: two sub-populations (Balding-Nichols, F = 0.05) crossed with sib-ships of 4, a phenotype with a sub-population shift and a
    polygenic part, every tested SNP null, no covariate for either (tests/_assoc_mixed_ref.py::structured_case, seed 2, shift 0.4, h2g 0.3; chosen on the CPU
    with the dense reference alone).  The reference's lambda_GC: plain OLS score test 2.156, mixed statistic (LOCO, 3 blocks) 0.977.  Without the
    feature there is no assoc_mixed, and assoc_linear is all a user has."""
    codes, y, _ = mr.structured_case(401, 1200, seed=2, shift=0.4, h2g=0.3)
    plink = mr.pack(codes)
    lin = mx.assoc_linear(plink, 1200, 401, y)
    lam_lin = mr.lambda_gc(lin.t)
    res = mx.assoc_mixed(plink, 1200, 401, y, chrom_bounds=EVEN)
    lam_mixed = mr.lambda_gc(res.zstat)
    print("lambda_GC: assoc_linear", lam_lin, "assoc_mixed", lam_mixed, "h2", res.h2, "gamma", res.gamma.ravel())
    assert lam_lin > 1.5 and abs(lam_lin - 2.156) <= 0.05              # the t statistic and the score statistic differ by O(z^2 / indiv)
    assert abs(lam_mixed - 0.977) <= 0.03 and 0.85 <= lam_mixed <= 1.15
    assert res.gamma.shape == (3, 1)


def test_host_and_device_operands_give_the_same_results(mx):
    import torch
    name = "256-n3-q2-estimated-loco-exact"
    c, ref = CASES[name], reference(name)
    _, plink, Y, W = data(c["indiv"], c["n"], c["q"], c["missing"])
    pd, Yd = torch.from_numpy(plink).cuda(), torch.from_numpy(np.ascontiguousarray(Y)).cuda()
    for p, y, on_device in ((pd, Y, True), (pd, Yd, True), (plink, Yd, False), (torch.from_numpy(plink), torch.from_numpy(np.ascontiguousarray(Y)), False)):
        res = mx.assoc_mixed(p, 1200, c["indiv"], y, W, chrom_bounds=c["bounds"], loco=True, calib_snps=60, exact_cutoff=1.0, seed=3, probes=16, tol=TOL)
        for a in res[:7]:
            assert (hasattr(a, "is_cuda") and a.is_cuda) if on_device else isinstance(a, np.ndarray)
        assert isinstance(res.h2, np.ndarray) and isinstance(res.gamma, np.ndarray) and isinstance(res.nobs, np.ndarray)
        check_scan(res, ref, f"plink on the {'device' if on_device else 'host'}, Y {type(y).__name__}")


def test_the_example_runs_at_its_default_size():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "gwas_mixed.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    assert run.returncode == 0, run.stdout[-3000:]
    lam = {}
    for line in run.stdout.splitlines():
        if line.startswith("lambda_GC"):
            lam[line.split()[1].rstrip(":")] = float(line.split()[-1])
    print(run.stdout[-1500:])
    # the dense reference on the example's default data: 2.273 and 1.040
    assert set(lam) == {"assoc_linear", "assoc_mixed"} and lam["assoc_linear"] > 1.5 and 0.85 <= lam["assoc_mixed"] <= 1.15
    assert "top hits" in run.stdout
