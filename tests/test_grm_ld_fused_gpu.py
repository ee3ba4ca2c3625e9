"""GRM / LD with the element-wise post-processing of the reference's binding (src/bindings/Julia/crossproduct.jl:83-152: two BLAS.ger!, the
affine shift and the scaling for the GRM; syr! and the division by sigma sigma^T for LD) FUSED into the crossproduct epilogue: the column sums and
the diagonal of M = X X^T come from the staged 2-bit matrix, not from three more passes over the result.  Checked against a dense numpy
restatement of those lines (the reference tests' own oracle: tests/crossproduct/test_grm.jl:114-141, test_ld.jl:68-80, tolerance stated here:
1e-12 relative, far inside the reference's 1e-4 / 0.1) and BIT FOR BIT against the unfused kernels (MXA_XPROD_FUSED_POST=0), for both engines,
host and device results, ragged sizes, PLINK and raw 2-bit input, and through the slab pipeline of a host result."""
import numpy as np
import pytest

import _ld_ref as ldref
from _util import Oracle, make_problem, pack_plink, synth_genotypes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


def _grm_ref(Z, f, do_scale):
    """crossproduct.jl:94-107, literally: M = Z Z^T; ger, ger, affine shift, scaling"""
    return _grm_map(Z @ Z.T, f, do_scale)


def _grm_map(M, f, do_scale):
    """crossproduct.jl:96-107 on a given crossproduct M"""
    n = M.shape[0]
    cs = M.sum(axis=0)
    M = M - np.outer(cs, np.ones(n)) / n - np.outer(np.ones(n), cs) / n + cs.sum() / n ** 2
    return M / (2 * np.sum(f * (1 - f))) if do_scale else M


def _ld_ref(Z, f, indiv):
    """crossproduct.jl:137-149"""
    return _ld_map(Z.T @ Z, f, indiv)


def _ld_map(M, f, indiv):
    """crossproduct.jl:139-149 on a given crossproduct M"""
    M = M - 4.0 * indiv * np.outer(f, f)
    s = np.sqrt(np.diag(M))
    return M / s[:, None] / s[None, :]


@pytest.mark.parametrize("snps,indiv", [(3000, 400), (777, 515), (130, 1031), (5000, 257)])
@pytest.mark.parametrize("engine", ["f4", "i8"])
def test_fused_grm_and_ld_equal_the_unfused_kernels_and_the_dense_restatement(mx, monkeypatch, snps, indiv, engine):
    monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
    prob = make_problem(snps, indiv, 1, seed=snps + indiv)
    Z = prob["Z"].astype(np.float64)          # indiv x snps, values 0 / 1 / 2 (no missings)
    f = prob["f"]
    cp = mx.crossproduct
    for do_scale in (True, False):
        monkeypatch.setenv("MXA_XPROD_FUSED_POST", "1")
        G = cp.grm(prob["plink_t"], snps, indiv, is_plink_format=True, do_scale=do_scale, allele_freq=f if do_scale else None)
        monkeypatch.setenv("MXA_XPROD_FUSED_POST", "0")
        G0 = cp.grm(prob["plink_t"], snps, indiv, is_plink_format=True, do_scale=do_scale, allele_freq=f if do_scale else None)
        assert np.array_equal(G, G0)
        assert np.array_equal(G, G.T)             # the maps are symmetric in (i, j) bit for bit
        ref = _grm_ref(Z, f, do_scale)
        assert np.abs(G - ref).max() <= 1e-12 * np.abs(ref).max()
    monkeypatch.setenv("MXA_XPROD_FUSED_POST", "1")
    R = cp.ld(prob["plink"], snps, indiv, is_plink_format=True, allele_freq=f)
    monkeypatch.setenv("MXA_XPROD_FUSED_POST", "0")
    R0 = cp.ld(prob["plink"], snps, indiv, is_plink_format=True, allele_freq=f)
    assert np.array_equal(R, R0, equal_nan=True)
    assert np.array_equal(R, R.T, equal_nan=True)
    ref = _ld_ref(Z, f, indiv)
    ok = np.isfinite(ref)                     # a monomorphic SNP has sigma = 0 in the reference too
    assert np.array_equal(np.isfinite(R), ok)
    assert np.abs(R[ok] - ref[ok]).max() <= 1e-11
    # ... and element by element: the bound derived from the map's own roundings (tests/_ld_ref.py), against the exact integer product and long double
    case = ldref.plain_case(prob["plink"], indiv, f)
    assert ok.all() and np.isfinite(case["b"]).all()
    ratio = ldref.worst_ratio(R, case["r"], case["b"])
    print(f"mxa_ld {snps}x{indiv} {engine}: worst |r - r_ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0, ratio


def test_fused_grm_device_resident_and_through_the_host_slab_pipeline(mx, monkeypatch):
    import torch
    dev = torch.device("cuda", 0)
    snps, indiv = 2100, 1290
    prob = make_problem(snps, indiv, 1, seed=8)
    f = prob["f"]
    cp = mx.crossproduct
    ref = _grm_ref(prob["Z"].astype(np.float64), f, True)
    Gd = cp.grm(torch.from_numpy(prob["plink_t"]).to(dev), snps, indiv, is_plink_format=True, do_scale=True, allele_freq=torch.from_numpy(f).to(dev))
    assert Gd.is_cuda
    monkeypatch.setenv("MXA_XPROD_SLAB_MB", "3")            # one tile row per chunk: six chunks, copied out while the next one computes
    Gh = cp.grm(prob["plink_t"], snps, indiv, is_plink_format=True, do_scale=True, allele_freq=f)
    monkeypatch.setenv("MXA_XPROD_NO_PIPELINE", "1")
    Gn = cp.grm(prob["plink_t"], snps, indiv, is_plink_format=True, do_scale=True, allele_freq=f)
    assert np.array_equal(Gd.cpu().numpy(), Gh) and np.array_equal(Gh, Gn)
    assert np.abs(Gh - ref).max() <= 1e-12 * np.abs(ref).max()
    Rh = cp.ld(prob["plink"], snps, indiv, is_plink_format=True, allele_freq=f)
    monkeypatch.delenv("MXA_XPROD_NO_PIPELINE")
    Rp = cp.ld(prob["plink"], snps, indiv, is_plink_format=True, allele_freq=f)
    assert np.array_equal(Rh, Rp, equal_nan=True)


def test_fused_grm_raw_two_bit_values_up_to_three(mx, monkeypatch):
    """is_plink_format = False: the packed fields are the values themselves, 3 included (the column sums and the diagonal must count 3 and 9)"""
    rng = np.random.default_rng(11)
    rows, k = 389, 1203
    V = rng.integers(0, 4, size=(rows, k)).astype(np.uint8)
    Vp = np.zeros((rows, (k + 3) // 4 * 4), dtype=np.uint8); Vp[:, :k] = V
    X = np.ascontiguousarray((Vp[:, 0::4] | (Vp[:, 1::4] << 2) | (Vp[:, 2::4] << 4) | (Vp[:, 3::4] << 6)).astype(np.uint8))
    Zf = V.astype(np.float64)
    f = rng.uniform(0.1, 0.5, size=k)
    cp = mx.crossproduct
    G = cp.grm(X, k, rows, is_plink_format=False, do_scale=True, allele_freq=f)
    monkeypatch.setenv("MXA_XPROD_FUSED_POST", "0")
    G0 = cp.grm(X, k, rows, is_plink_format=False, do_scale=True, allele_freq=f)
    assert np.array_equal(G, G0)
    ref = _grm_ref(Zf, f, True)
    assert np.abs(G - ref).max() <= 1e-12 * np.abs(ref).max()


# ---------------------------------------------------------------------------------------------------- PLINK input with missing codes
def _problem_with_missing_in_last_bytes(snps, indiv, seed, frac=0.05):
    """~5 % missing codes (01), and more in the LAST byte of rows of both orientations: in the individual-major matrix (GRM input) the last SNP of
    every 7th individual, in the SNP-major matrix (LD input) the last individual of every 5th SNP.  Under the reference's byte table such a byte is
    0xFF, four 3s: the padding fields of a ragged last byte (snps % 4, indiv % 4 != 0) become 3s as well, and the product counts them."""
    Z, miss = synth_genotypes(snps, indiv, seed, missing_frac=frac)
    miss[::7, snps - 1] = True
    miss[indiv - 1, ::5] = True
    Zeff = np.where(miss, 0, Z).astype(np.int8)
    return dict(snps=snps, indiv=indiv, plink=pack_plink(np.ascontiguousarray(Z.T), np.ascontiguousarray(miss.T)), plink_t=pack_plink(Z, miss),
                f=Zeff.astype(np.float64).mean(axis=0) / 2.0, Z=Zeff)


def _dense_with_quirk(o, prob):
    """the dense restatement of crossproduct.jl:83-152 on Oracle.crossprod_i32, which reads a byte with a missing pair as 0xFF (four 3s)"""
    snps, indiv = prob["snps"], prob["indiv"]
    Mg = o.crossprod_i32(prob["plink_t"], snps, True).astype(np.float64)     # indiv x indiv
    Ml = o.crossprod_i32(prob["plink"], indiv, True).astype(np.float64)      # snps x snps
    return Mg, Ml


def _check_grm_ld(cp, monkeypatch, prob, Mg, Ml, to=lambda a: a, back=lambda a: a):
    """fused == unfused bit for bit, both == the dense restatement (1e-12 of max|G|, 1e-11 for LD); returns the fused results"""
    snps, indiv, f = prob["snps"], prob["indiv"], prob["f"]
    X_t, X, fd = to(prob["plink_t"]), to(prob["plink"]), to(f)
    out = {}
    for do_scale in (True, False):
        Gs = []
        for fused in ("1", "0"):
            monkeypatch.setenv("MXA_XPROD_FUSED_POST", fused)
            Gs.append(back(cp.grm(X_t, snps, indiv, is_plink_format=True, do_scale=do_scale, allele_freq=fd if do_scale else None)))
        assert np.array_equal(Gs[0], Gs[1]), ("GRM fused != unfused", do_scale)
        assert np.array_equal(Gs[0], Gs[0].T), ("GRM not symmetric", do_scale)
        ref = _grm_map(Mg, f, do_scale)
        assert np.abs(Gs[0] - ref).max() <= 1e-12 * np.abs(ref).max(), do_scale
        out[do_scale] = Gs[0]
    Rs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("MXA_XPROD_FUSED_POST", fused)
        Rs.append(back(cp.ld(X, snps, indiv, is_plink_format=True, allele_freq=fd)))
    monkeypatch.delenv("MXA_XPROD_FUSED_POST")
    assert np.array_equal(Rs[0], Rs[1], equal_nan=True), "LD fused != unfused"
    assert np.array_equal(Rs[0], Rs[0].T, equal_nan=True), "LD not symmetric"
    ref = _ld_map(Ml, f, indiv)
    ok = np.isfinite(ref)
    assert np.array_equal(np.isfinite(Rs[0]), ok)
    assert np.abs(Rs[0][ok] - ref[ok]).max() <= 1e-11
    out["ld"] = Rs[0]
    return out


@pytest.mark.parametrize("snps,indiv", [(1001, 515), (2022, 1030), (779, 1285)])     # K % 4 = 1, 2, 3 for the GRM (snps) and 3, 2, 1 for LD (indiv)
@pytest.mark.parametrize("engine", ["default", "i8"])
def test_fused_grm_and_ld_with_missing_codes_in_ragged_last_bytes(mx, monkeypatch, snps, indiv, engine):
    """The statistics the fused map uses (k_x_colsum, k_x_rowstats, k_x_finish_stats) must count the 3s of a 0xFF byte -- padding fields included --
    exactly as the product does: host input and output"""
    if engine == "i8":
        monkeypatch.setenv("MXA_XPROD_ENGINE", "i8")
    prob = _problem_with_missing_in_last_bytes(snps, indiv, seed=snps * 7 + indiv)
    Mg, Ml = _dense_with_quirk(Oracle(), prob)
    Zf = prob["Z"].astype(np.float64)
    assert (Mg > Zf @ Zf.T).any() and (np.diag(Ml) > np.diag(Zf.T @ Zf)).any()    # the 3s are there: more than the genotypes alone
    _check_grm_ld(mx.crossproduct, monkeypatch, prob, Mg, Ml)


def test_fused_grm_and_ld_with_missing_codes_device_resident_and_through_the_host_ring(mx, monkeypatch):
    """the same data with every operand in HBM, and a host result produced slab by slab through the ring of device buffers (MXA_XPROD_HOST_RING=2,
    small slabs: the ring wraps several times); all three bit-identical"""
    import torch
    dev = torch.device("cuda", 0)
    prob = _problem_with_missing_in_last_bytes(2022, 1030, seed=3)
    Mg, Ml = _dense_with_quirk(Oracle(), prob)
    cp = mx.crossproduct
    dres = _check_grm_ld(cp, monkeypatch, prob, Mg, Ml, to=lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev), back=lambda t: t.cpu().numpy())
    monkeypatch.setenv("MXA_XPROD_SLAB_MB", "3")
    monkeypatch.setenv("MXA_XPROD_HOST_RING", "2")
    hres = _check_grm_ld(cp, monkeypatch, prob, Mg, Ml)
    for key in (True, False, "ld"):
        assert np.array_equal(dres[key], hres[key], equal_nan=True), key
