"""Windowed LD at BASELINE config 2's full size -- the point of the feature: 1 000 000 SNPs x 50 000 individuals, window 1023.  mxa_ld's result would be
8 TB; mxa_ld_band writes the 8.2 GB band into a device result and mxa_ld_scores the 1 000 000 scores, over 19 525 tiles.  Sampled SNPs -- the first one,
SNPs on both sides of a 256-SNP tile edge, interior ones, and SNPs of the last `window` (tail zeros) -- are compared with a dense restatement of
crossproduct.jl:137-149 computed here from the extracted rows (exact integer crossproduct in fp64, f from the data) at 1e-12 relative, and the scores with
math.fsum of the squares of the band just produced under the bound of any summation order, m 2^-53 sum|t| (tests/test_ld_band_gpu.py).
A module of its own: nothing else may hold device memory beside the operand, its staged copy and the band."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SNPS, INDIV, WINDOW = 1_000_000, 50_000, 1023
SAMPLES = [0, 255, 256, 300_001, 767_999, SNPS - WINDOW - 1, SNPS - WINDOW, SNPS - 513, SNPS - 1]


def _genotypes(torch, rows, cols, seed, dev):
    """SNP-major PLINK rows (rows x ceil(cols/4) bytes), Binomial(2, p_s) with p_s ~ U(0.1, 0.6) per SNP (row), no missings"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rb = (cols + 3) // 4
    out = torch.empty((rows, rb), dtype=torch.uint8, device=dev)
    w = torch.tensor([1, 4, 16, 64], dtype=torch.uint8, device=dev)
    chunk = max(1, (256 << 20) // (4 * rb))
    for r0 in range(0, rows, chunk):
        r1 = min(rows, r0 + chunk)
        p = (torch.rand(r1 - r0, device=dev, generator=g) * 0.5 + 0.1)[:, None]
        q0, q1 = (1.0 - p) ** 2, (1.0 - p) ** 2 + 2.0 * p * (1.0 - p)
        u = torch.rand((r1 - r0, 4 * rb), device=dev, generator=g)
        code = (u >= q0).to(torch.uint8) * 2 + (u >= q1).to(torch.uint8)        # 0 -> 00, 1 -> 10, 2 -> 11
        code[:, cols:] = 0
        out[r0:r1] = (code.view(r1 - r0, rb, 4) * w).sum(dim=2, dtype=torch.uint8)
        del u, code
    return out


def _values(torch, B):
    """PLINK bytes (rows x nb, device) -> genotype values (rows x 4 nb, uint8): 00 -> 0, 10 -> 1, 11 -> 2"""
    f = torch.stack([(B >> (2 * q)) & 3 for q in range(4)], dim=2).view(B.shape[0], -1)
    return (f >> 1) + ((f >> 1) & f & 1)


@pytest.fixture(scope="module")
def full():
    import torch
    import miraculix_amd as mx
    mx.load_shared_library()
    torch.cuda.empty_cache()
    dev = torch.device("cuda", 0)
    X = _genotypes(torch, SNPS, INDIV, 62, dev)                                    # 12.5 GB
    t = torch.empty(SNPS, dtype=torch.int64, device=dev)                           # allele counts per SNP, exact
    for r0 in range(0, SNPS, 8192):
        t[r0:r0 + 8192] = _values(torch, X[r0:r0 + 8192]).sum(dim=1, dtype=torch.int64)
    f = t.to(torch.float64) / (2.0 * INDIV)                                        # from the data
    band = mx.crossproduct.ld_band(X, SNPS, INDIV, WINDOW, kind="r", is_plink_format=True, allele_freq=f)      # 8.2 GB, device
    scores = mx.crossproduct.ld_scores(X, SNPS, INDIV, WINDOW, is_plink_format=True, allele_freq=f)
    torch.cuda.synchronize()
    yield dict(torch=torch, dev=dev, X=X, f=f, band=band, scores=scores, mx=mx)
    del X, band, scores, t, f
    torch.cuda.empty_cache()


def test_ld_band_full_sampled_snps_against_the_dense_restatement(full):
    torch, X, band = full["torch"], full["X"], full["band"]
    assert band.is_cuda and tuple(band.shape) == (SNPS, WINDOW + 1)
    f = full["f"].cpu().numpy()
    assert any(i % 256 == 255 for i in SAMPLES) and any(i >= SNPS - WINDOW for i in SAMPLES) and 0 in SAMPLES and len(SAMPLES) >= 8
    for i in SAMPLES:
        hi = min(SNPS, i + WINDOW + 1)
        V = _values(torch, X[i:hi])[:, :INDIV].to(torch.float64)                  # the window's rows, values 0 / 1 / 2
        M = (V @ V[0]).cpu().numpy()                                               # integers < 2^53: exact
        D = (V * V).sum(dim=1).cpu().numpy()
        del V
        fw = f[i:hi]
        sig = np.sqrt(D - 4.0 * INDIV * fw * fw)
        ref = (M - 4.0 * INDIV * fw[0] * fw) / sig[0] / sig
        got = band[i].cpu().numpy()
        assert np.isfinite(ref).all()
        assert np.abs(got[: hi - i] - ref).max() <= 1e-12 * np.abs(ref).max(), i
        assert np.all(got[hi - i:] == 0.0), i                                     # i + d >= snps
        assert got[0] == 1.0 or abs(got[0] - 1.0) <= 4 * U, i


def test_ld_scores_full_sampled_snps_against_the_host_sum_of_the_band(full):
    torch, band = full["torch"], full["band"]
    scores = full["scores"]
    assert scores.is_cuda and tuple(scores.shape) == (SNPS,)
    assert bool(torch.isfinite(scores).all())
    m = 2 * WINDOW + 1
    d = torch.arange(1, WINDOW + 1, device=full["dev"])
    for i in SAMPLES:
        right = band[i, : min(WINDOW + 1, SNPS - i)]                               # r(i, i + d), d >= 0
        dl = d[: min(WINDOW, i)]
        left = band[i - dl, dl]                                                    # r(i - d, i), d >= 1
        r = torch.cat([right, left]).cpu().numpy()
        t = r * r
        ref, mag = math.fsum(t), math.fsum(np.abs(t))
        err = abs(float(scores[i]) - ref)
        print(f"score {i}: {float(scores[i])!r}, |err| / bound = {err / (m * U * mag):.3f}")
        assert err <= m * U * mag, (i, err / (m * U * mag))


def test_ld_scores_full_are_reproducible(full):
    mx, torch = full["mx"], full["torch"]
    again = mx.crossproduct.ld_scores(full["X"], SNPS, INDIV, WINDOW, is_plink_format=True, allele_freq=full["f"])
    assert torch.equal(again, full["scores"])
