"""The reference's own test grids for the integer crossproduct and the GRM (tests/crossproduct/test_grm.jl:114-157), run in full, each against a
product that this project's kernels do not compute (torch fp64 GEMMs on the unpacked values):

  * "Correctness in uneven dimensions": K in {953, 10251} SNPs x {752, 5343, 12433} individuals, both engines (default, MXA_XPROD_ENGINE=i8),
    PLINK codes and raw 2-bit fields (values 0..3), host input and host output -- bit-exact against Z Z^T in fp64, exact because every partial
    sum is an integer below 2^53 (at most 9 * 10251).
  * "Correctness for 2bit simulated data": raw fields 0..2 at {1e4, 5e4, 1e5} SNPs x {2e3, 15e3} individuals, f from the data, do_scale: the uncentred
    crossproduct bit-exact, the GRM against the CENTRE-FIRST product (Z - 2f)(Z - 2f)^T / (2 sum f(1-f)) of the reference's test (the library
    multiplies first and centres in its epilogue: a different computation), element-wise, and the fused epilogue bit-identical to the unfused passes."""
import numpy as np
import pytest

from _util import pack_plink

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


def _pack_raw(V):
    """rows x k values 0..3 -> rows x ceil(k/4) bytes, field q of byte b = value 4 b + q (low bits first), padding fields zero"""
    rows, k = V.shape
    Vp = np.zeros((rows, (k + 3) // 4 * 4), np.uint8)
    Vp[:, :k] = V
    return np.ascontiguousarray(Vp[:, 0::4] | (Vp[:, 1::4] << 2) | (Vp[:, 2::4] << 4) | (Vp[:, 3::4] << 6))


@pytest.mark.parametrize("k", [953, 10251])
@pytest.mark.parametrize("rows", [752, 5343, 12433])
def test_uneven_grid_bit_exact_both_engines_both_formats(mx, monkeypatch, k, rows):
    """test_grm.jl:143-157 (snp_crossprod at uneven sizes; the reference accepts sum|ANS - D| < 1e-4, here: equal)"""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1000 * k + rows)
    Z = rng.integers(0, 3, size=(rows, k), dtype=np.int8)             # genotypes 0/1/2 -> PLINK codes 00/10/11
    V = rng.integers(0, 4, size=(rows, k), dtype=np.int8)             # raw 2-bit fields, 3 included
    for fmt, vals, X in (("plink", Z, pack_plink(Z)), ("raw", V, _pack_raw(V))):
        Vd = torch.from_numpy(vals).to(dev).to(torch.float64)
        ref = Vd @ Vd.t()                                              # exact: integer partial sums < 2^53
        del Vd
        for engine in ("default", "i8"):
            if engine == "i8":
                monkeypatch.setenv("MXA_XPROD_ENGINE", "i8")
            else:
                monkeypatch.delenv("MXA_XPROD_ENGINE", raising=False)
            M = np.full((rows, rows), -1.0)
            mx.crossproduct.snp_crossprod(X, k, rows, is_snpmajor=False, is_plink_format=fmt == "plink", out=M)   # host in, host out
            assert torch.equal(torch.from_numpy(M).to(dev), ref), (fmt, engine)
            del M
        del ref
    monkeypatch.delenv("MXA_XPROD_ENGINE", raising=False)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("snps", [10_000, 50_000, 100_000])
@pytest.mark.parametrize("indiv", [2_000, 15_000])
def test_simulated_grm_grid_against_the_centre_first_product(mx, monkeypatch, snps, indiv):
    """test_grm.jl:114-139.  Raw fields 0..2 (is_plink_format = false), individual-major on the device, f = column means / 2.

    Bound, per element: |G - G_ref| <= 3 K 2^-53 (|Zc|^T |Zc|)_ij / (2 sum f(1-f)), Zc = Z - 2f.  One K 2^-53 for the fp64 dot products of the
    reference (gamma_K of a K-term sum of products, any order), one for the two K-term sums of f(1-f) that form the scale (the relative difference
    of the two scales times |G_ij| <= (|Zc|^T|Zc|)_ij / scale), one for the rounding of Zc and the library's own few roundings of its map on exact
    integers (the uncentred M, the column sums, their total: ~6 roundings at magnitude <= 3 K, far below K 2^-53 (|Zc|^T|Zc|)_ij ~ 0.3 K^2 2^-53)."""
    import torch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(snps + indiv)
    Z8 = torch.randint(0, 3, (indiv, snps), dtype=torch.uint8, device=dev, generator=g)
    pad = (-snps) % 4
    Zp = torch.nn.functional.pad(Z8, (0, pad)).view(indiv, -1, 4)
    X = (Zp[:, :, 0] | (Zp[:, :, 1] << 2) | (Zp[:, :, 2] << 4) | (Zp[:, :, 3] << 6)).contiguous()   # indiv x ceil(snps/4)
    del Zp
    Zf = Z8.to(torch.float64)
    del Z8
    cp = mx.crossproduct
    M = cp.snp_crossprod(X, snps, indiv, is_snpmajor=False, is_plink_format=False)
    assert M.is_cuda and torch.equal(M, Zf @ Zf.t())                  # uncentred: exact integers
    del M
    f = Zf.mean(dim=0) / 2.0                                           # from the data, as the reference test does
    monkeypatch.setenv("MXA_XPROD_FUSED_POST", "1")
    G = cp.grm(X, snps, indiv, is_plink_format=False, do_scale=True, allele_freq=f)
    monkeypatch.setenv("MXA_XPROD_FUSED_POST", "0")
    G0 = cp.grm(X, snps, indiv, is_plink_format=False, do_scale=True, allele_freq=f)
    monkeypatch.delenv("MXA_XPROD_FUSED_POST")
    assert torch.equal(G, G0), "fused epilogue differs from the unfused passes"
    assert torch.equal(G, G.t()), "GRM not symmetric"
    del G0
    scale = 2.0 * float((f * (1.0 - f)).sum())
    Zf.sub_(2.0 * f[None, :])                                          # Zc = Z - 2f, in place
    err = (G - (Zf @ Zf.t()) / scale).abs_()
    Zf.abs_()
    bound = (Zf @ Zf.t()).mul_(3.0 * snps * U / scale)
    worst = float((err / bound).max())
    assert worst <= 1.0, worst
    del Zf, G, err, bound, X
    torch.cuda.empty_cache()
