"""The GRM at BASELINE config 3's full size: mxa_grm on 500 000 SNPs x 100 000 individuals into a device-resident 80 GB result, do_scale, f from the
data -- the fused GRM map in the default (gang) form of the crossproduct over 76 k tiles, the u64 row statistics over 500 000 SNPs, and a total of
the column sums above 2^53.  tests/test_fullsize_configs_gpu.py checks the bare crossproduct at this size; this module checks the map.  The map is
restated from quantities computed here, independently of the library: the column sums t of X with exact int64 torch ops, the column sums of
M = X X^T as cs_r = x_r . t (exact int64), their total as sum t_s^2 (exact, a Python int), the crossproduct of sampled rows by Oracle.crossprod_i32.
A module of its own: nothing else may hold device memory while the 80 GB result lives."""
import numpy as np
import pytest

from _util import Oracle

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SNPS, INDIV = 500_000, 100_000


def _genotypes(torch, rows, cols, seed, dev):
    """individual-major PLINK rows (rows x ceil(cols/4) bytes), Binomial(2, p_s) with p_s ~ U(0.55, 0.95) per SNP (column), no missings: allele
    frequencies this high make sum_s t_s^2 ~ 1.2e16 > 2^53 (with bench.py's p ~ U(0.1, 0.6) it is ~2.9e15)"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rb = (cols + 3) // 4
    out = torch.empty((rows, rb), dtype=torch.uint8, device=dev)
    p = torch.nn.functional.pad(torch.rand(cols, device=dev, generator=g) * 0.4 + 0.55, (0, 4 * rb - cols))[None, :]
    q0, q1 = (1.0 - p) ** 2, (1.0 - p) ** 2 + 2.0 * p * (1.0 - p)
    w = torch.tensor([1, 4, 16, 64], dtype=torch.uint8, device=dev)
    chunk = max(1, (256 << 20) // (4 * rb))
    for r0 in range(0, rows, chunk):
        r1 = min(rows, r0 + chunk)
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
    X = _genotypes(torch, INDIV, SNPS, 61, dev)                                   # 12.5 GB
    t = torch.zeros(4 * X.shape[1], dtype=torch.int64, device=dev)                 # t_s = sum over individuals of x_is, exact
    for r0 in range(0, INDIV, 2048):
        t += _values(torch, X[r0:r0 + 2048]).sum(dim=0, dtype=torch.int64)
    t = t[:SNPS].contiguous()
    f = t.to(torch.float64) / (2.0 * INDIV)                                        # from the data
    G = mx.crossproduct.grm(X, SNPS, INDIV, is_plink_format=True, do_scale=True, allele_freq=f)   # 80 GB, device
    torch.cuda.synchronize()
    yield dict(torch=torch, dev=dev, X=X, t=t, f=f, G=G)
    del X, G, t, f
    torch.cuda.empty_cache()


def _scale_and_total(S):
    t = S["t"].cpu().numpy().astype(object)
    tot = int((t * t).sum())                                                       # sum_r cs_r = sum_s t_s^2, exact
    f = S["f"].cpu().numpy().astype(np.longdouble)
    return tot, 2 * (f * (1 - f)).sum()


def test_grm_full_exact_symmetry_and_row_sums(full):
    """G = P M P / c (P = I - 1 1^T / n) has zero row sums.  Per element the library rounds ~8 times at magnitude
    mag_ij = M_ij + cs_i/n + cs_j/n + tot/n^2, whose row sum is 2 (cs_i + tot/n) <= 2 (2 sum t + tot/n) (x <= 2); its fp64 total of the n column sums
    errs by <= (n - 1) u tot, i.e. u tot over a row; the scale errs relatively (common to the row: no effect on a zero sum); torch's fp64 row sum errs by
    <= n u sum_j |G_ij|.  Bound: (16 u (2 sum t + tot/n) + u tot) / c + n u sum_j |G_ij|."""
    torch, G = full["torch"], full["G"]
    n = INDIV
    step = 2048
    for a in range(0, n, step):
        b = min(n, a + step)
        assert torch.equal(G[a:b, :], G[:, a:b].t()), (a, b)                      # exact symmetry, panel by panel
    tot, c = _scale_and_total(full)
    assert tot > 2 ** 53                                                           # the total the map uses is not an exact double
    sum_t = int(full["t"].sum())
    rs = torch.empty(n, dtype=torch.float64, device=full["dev"])
    ra = torch.empty(n, dtype=torch.float64, device=full["dev"])
    for a in range(0, n, step):
        rs[a:a + step] = G[a:a + step].sum(dim=1)
        ra[a:a + step] = G[a:a + step].abs().sum(dim=1)
    bound = float((16 * U * (2 * sum_t + tot / n) + U * tot) / c) + n * U * ra
    assert bool(torch.isfinite(rs).all())
    worst = float((rs.abs() / bound).max())
    assert worst <= 1.0, (worst, float(rs.abs().max()))
    d = torch.diagonal(G)
    assert float(d.min()) > 0.0                                                    # a GRM's diagonal: 1 + inbreeding, positive


def test_grm_full_sampled_tiles_against_the_map_of_the_exact_product(full):
    """eight 256 x 256 tiles: the first and the last (ragged, 160 rows) diagonal tiles, tiles in the far corner whose element offsets exceed 2^32,
    random interior tiles.  Reference: the map of crossproduct.jl:94-107 in long double on Oracle.crossprod_i32 of the extracted rows, with cs and
    the total exact.  Bound per element: 8 u mag_ij / c (the library's ~8 roundings of the map), + u tot / (n c) (its fp64 total of n column sums:
    <= (n - 1) u tot, divided by n^2), + 2 K u |G_ij| (its fp64 sum of K terms f (1 - f) for the scale against the long-double one)."""
    torch, G, X, dev = full["torch"], full["G"], full["X"], full["dev"]
    n, k = INDIV, SNPS
    o = Oracle()
    tot, c = _scale_and_total(full)
    tot_l = np.longdouble(tot)
    nb = (n + 255) // 256
    rng = np.random.default_rng(17)
    tiles = [(0, 0), (nb - 1, nb - 1), (0, nb - 1), (nb - 2, nb - 1), (150, 330)]
    while len(tiles) < 8:
        i, j = sorted(rng.integers(0, nb, 2).tolist())
        tiles.append((int(i), int(j)))
    assert any(i * 256 * n + j * 256 > 2 ** 32 for i, j in tiles)
    t = full["t"]
    for ti, tj in tiles:
        ri = np.arange(ti * 256, min(n, ti * 256 + 256))
        rj = np.arange(tj * 256, min(n, tj * 256 + 256))
        rows = np.concatenate([ri, rj]) if ti != tj else ri
        sub_d = X.index_select(0, torch.as_tensor(rows, device=dev))
        cs = (_values(torch, sub_d)[:, :k].to(torch.int64) * t[None, :]).sum(dim=1).cpu().numpy()   # cs_r = x_r . t, exact int64
        Mt = o.crossprod_i32(np.ascontiguousarray(sub_d.cpu().numpy()), k, True).astype(np.longdouble)
        del sub_d
        csl = cs.astype(np.longdouble)
        ref = (Mt - csl[:, None] / n - csl[None, :] / n + tot_l / (np.longdouble(n) * n)) / c
        mag = (Mt + csl[:, None] / n + csl[None, :] / n + tot_l / (np.longdouble(n) * n)) / c
        if ti != tj:
            ref, mag = ref[: len(ri), len(ri):], mag[: len(ri), len(ri):]
        ref, mag = ref.astype(np.float64), mag.astype(np.float64)
        bound = 8 * U * mag + U * float(tot_l / (np.longdouble(n) * c)) + 2 * k * U * np.abs(ref)
        # G is symmetric and column-major in the C ABI's view: G[r, s] = M-map at (r, s) either way
        got = G[ri[0]:ri[-1] + 1, rj[0]:rj[-1] + 1].cpu().numpy()
        ratio = float((np.abs(got - ref) / bound).max())
        assert ratio <= 1.0, (ti, tj, ratio)
        assert cs.max() > 2 ** 32                                                  # the u64 statistics are needed
