"""Host-side mirror of the reference's Julia module `miraculix.crossproduct`
(src/bindings/Julia/crossproduct.jl:44-152): snp_crossprod, grm, ld over the C symbol snp_multiply_gpu."""
import numpy as np

from . import lib as _lib


def _zeros_like(plink, *shape):
    """the result of an entry: float64 zeros of `shape`, numpy or -- for a torch input -- a tensor on the input's device"""
    if _lib.is_torch_tensor(plink):
        import torch
        return torch.zeros(shape, dtype=torch.float64, device=plink.device)
    return np.zeros(shape, dtype=np.float64)


def _check(rc, entry):
    if rc != 0:
        raise RuntimeError(f"{entry} failed: " + _lib.last_error()[1])


def snp_crossprod(plink, snps, indiv, is_snpmajor, is_plink_format=False, out=None):
    """crossproduct.jl:44-64.  plink: 2-bit matrix, one row per output index: for is_snpmajor=False `indiv` rows of
    ceil(snps/4) bytes (result indiv x indiv), for is_snpmajor=True `snps` rows of ceil(indiv/4) bytes (result snps x snps).
    numpy uint8 (host) or torch uint8 tensor (host/device).  Returns the full symmetric Float64 matrix (numpy, or a torch
    tensor on the input's device)."""
    if is_snpmajor:
        nrow, ncol = indiv, snps
    else:
        nrow, ncol = snps, indiv
    nbytes = int(np.prod(plink.shape))
    if nbytes != ncol * ((nrow + 3) // 4):
        raise ValueError(f"Matrix has wrong dimensions: {tuple(plink.shape)}")
    L = _lib.check_library_handle()
    M = out if out is not None else _zeros_like(plink, ncol, ncol)
    _check(L.snp_multiply_gpu(_lib.ptr(plink), int(nrow), int(ncol), _lib.ptr(M), bool(is_plink_format)), "snp_multiply_gpu")
    return M


def snp_crossprod_panel(plink, inner, n_out, col_begin, col_end, upper_only=False, is_plink_format=False, out=None):
    """Additive (C entry mxa_snp_multiply_panel): columns [col_begin, col_end) of the symmetric n_out x n_out crossproduct of the
    2-bit matrix `plink` (n_out rows of ceil(inner/4) bytes).  Returns the panel as a tensor/array P of shape
    (col_end - col_begin, n_out) with P[c, r] = M[r, col_begin + c] -- the contiguous slab of the column-major result.
    upper_only: only rows [0, col_end) are computed (zeros below)."""
    if int(np.prod(plink.shape)) != n_out * ((inner + 3) // 4):
        raise ValueError(f"Matrix has wrong dimensions: {tuple(plink.shape)}")
    w = col_end - col_begin
    L = _lib.check_library_handle()
    P = out if out is not None else _zeros_like(plink, w, n_out)
    _check(L.mxa_snp_multiply_panel(_lib.ptr(plink), int(inner), int(n_out), int(col_begin), int(col_end), int(bool(upper_only)), _lib.ptr(P), int(n_out),
                                    int(bool(is_plink_format))), "mxa_snp_multiply_panel")
    return P


def grm(plink_transposed, snps, indiv, is_plink_format=False, do_scale=True, allele_freq=None):
    """crossproduct.jl:83-110; maths docs/grm.md:5-12.  G = P Z Z^T P^T / (2 sum f(1-f)): the crossproduct and the rank-1
    centring / scaling all run on the device (C entry mxa_grm); only the finished G crosses PCIe when inputs are host arrays."""
    if do_scale and (allele_freq is None or len(allele_freq) != snps):
        raise ValueError(f"Allele frequencies need to be equal to length of SNPs {snps}.")
    if int(np.prod(plink_transposed.shape)) != indiv * ((snps + 3) // 4):
        raise ValueError(f"Matrix has wrong dimensions: {tuple(plink_transposed.shape)}")
    L = _lib.check_library_handle()
    G = _zeros_like(plink_transposed, indiv, indiv)
    f = allele_freq
    if f is not None and not _lib.is_torch_tensor(f):
        f = np.ascontiguousarray(f, dtype=np.float64)
    _check(L.mxa_grm(_lib.ptr(plink_transposed), int(snps), int(indiv), _lib.ptr(G), int(bool(is_plink_format)), int(bool(do_scale)), _lib.ptr(f)), "mxa_grm")
    return G


def ld(plink, snps, indiv, is_plink_format=False, allele_freq=None):
    """crossproduct.jl:128-152: LD correlation from the SNP x SNP crossproduct, on the device (C entry mxa_ld)."""
    if allele_freq is None or len(allele_freq) != snps:
        raise ValueError(f"Allele frequencies need to be equal to length of SNPs {snps}.")
    if int(np.prod(plink.shape)) != snps * ((indiv + 3) // 4):
        raise ValueError(f"Matrix has wrong dimensions: {tuple(plink.shape)}")
    L = _lib.check_library_handle()
    R = _zeros_like(plink, snps, snps)
    f = allele_freq if _lib.is_torch_tensor(allele_freq) else np.ascontiguousarray(allele_freq, dtype=np.float64)
    _check(L.mxa_ld(_lib.ptr(plink), int(snps), int(indiv), _lib.ptr(R), int(bool(is_plink_format)), _lib.ptr(f)), "mxa_ld")
    return R


def ld_band_tiles(snps, window):
    """The tile plan of the windowed LD entries, restated: the 256 x 256 tiles (I, J), I <= J, that hold an element (i, j) with 0 <= j - i <= window.
    Tile (I, J) holds the offsets j - i in [256 (J - I) - 255, 256 (J - I) + 255], so it meets the band iff J - I <= (window + 255) // 256 = ceil(window / 256)."""
    nb = (snps + 255) // 256
    ndiag = (window + 255) // 256
    return [(i, j) for i in range(nb) for j in range(i, min(nb, i + ndiag + 1))]


def _ld_window_args(plink, snps, indiv, window, allele_freq):
    if allele_freq is None or len(allele_freq) != snps:
        raise ValueError(f"Allele frequencies need to be equal to length of SNPs {snps}.")
    if int(np.prod(plink.shape)) != snps * ((indiv + 3) // 4):
        raise ValueError(f"Matrix has wrong dimensions: {tuple(plink.shape)}")
    if not 0 <= int(window) < snps:
        raise ValueError(f"Window needs to be in [0, {snps}): {window}")
    return allele_freq if _lib.is_torch_tensor(allele_freq) else np.ascontiguousarray(allele_freq, dtype=np.float64)


def ld_band(plink, snps, indiv, window, kind="r", is_plink_format=False, allele_freq=None):
    """Additive (C entry mxa_ld_band): the band of ld()'s R within `window` SNPs of the diagonal, shape (snps, window + 1) with out[i, d] = R(i, i + d)
    (0.0 where i + d >= snps) -- LAPACK's lower symmetric band storage, column by column.  kind "r" or "r2".  The snps x snps matrix is never formed."""
    if kind not in ("r", "r2"):
        raise ValueError(f"kind needs to be 'r' or 'r2': {kind!r}")
    f = _ld_window_args(plink, snps, indiv, window, allele_freq)
    L = _lib.check_library_handle()
    B = _zeros_like(plink, snps, int(window) + 1)
    _check(L.mxa_ld_band(_lib.ptr(plink), int(snps), int(indiv), int(window), _lib.ptr(B), int(window) + 1, 1 if kind == "r2" else 0, int(bool(is_plink_format)), _lib.ptr(f)), "mxa_ld_band")
    return B


def ld_scores(plink, snps, indiv, window, adjust=False, is_plink_format=False, allele_freq=None):
    """Additive (C entry mxa_ld_scores): LD scores l_i = sum over |i - j| <= window of r_ij^2 (adjust: of r^2 - (1 - r^2) / (indiv - 2), the estimator of
    LD-score regression), shape (snps,).  Neither the matrix nor the band is written to memory; the sums run in a fixed order (bitwise reproducible)."""
    f = _ld_window_args(plink, snps, indiv, window, allele_freq)
    if adjust and indiv < 3:
        raise ValueError(f"The adjusted estimator needs at least 3 individuals: {indiv}")
    L = _lib.check_library_handle()
    S = _zeros_like(plink, snps)
    _check(L.mxa_ld_scores(_lib.ptr(plink), int(snps), int(indiv), int(window), _lib.ptr(S), int(bool(adjust)), int(bool(is_plink_format)), _lib.ptr(f)), "mxa_ld_scores")
    return S


# ---- pairwise-complete windowed LD (data with missing genotypes): C entries mxa_ld_band_pairwise / mxa_ld_scores_pairwise
PAIRWISE_PLANES = {"Z": 0, "M": 1, "A": 2}                    # planes of the stacked operand: allele count (missing as 0), present, code 11
# the six products of a band tile in slot order: N, Sxy, Sx, Sy, sum a_i m_j, sum m_i a_j -- (plane of the I rows, plane of the J rows)
PAIRWISE_PAIRS = (("M", "M"), ("Z", "Z"), ("Z", "M"), ("M", "Z"), ("A", "M"), ("M", "A"))
PAIRWISE_SLOT_BYTES = 256 * 256 * 4                           # one int32 count tile


def ld_pairwise_group_rows(snps, window, scratch_mb=2048, pairs=6):
    """Tile rows per group of the pairwise entries: as many as keep the count scratch (pairs slots of 256 KiB per band tile, a tile row holding up to
    min(nb, ceil(window / 256) + 1) tiles) under scratch_mb MiB -- one tile row at least, the whole band at most."""
    nb = (snps + 255) // 256
    row_tiles = min(nb, (window + 255) // 256 + 1)
    return max(1, min(nb, (scratch_mb << 20) // (row_tiles * pairs * PAIRWISE_SLOT_BYTES)))


def ld_pairwise_tiles(snps, window, group):
    """The tile plan of the pairwise entries, restated: the band tiles of ld_band_tiles in groups of `group` tile rows; per band tile (I, J) six entries
    (x, y, slot) over the stacked operand of 3 nb row blocks, x = plane_a * nb + I, y = plane_b * nb + J for the pairs of PAIRWISE_PAIRS, written to the
    scratch slots 6 q .. 6 q + 5 of the tile's position q within its group.  Returns the list of groups."""
    nb = (snps + 255) // 256
    ndiag = (window + 255) // 256
    groups = []
    for i_lo in range(0, nb, group):
        entries, q = [], 0
        for i in range(i_lo, min(nb, i_lo + group)):
            for j in range(i, min(nb, i + ndiag + 1)):
                for k, (pa, pb) in enumerate(PAIRWISE_PAIRS):
                    entries.append((PAIRWISE_PLANES[pa] * nb + i, PAIRWISE_PLANES[pb] * nb + j, 6 * q + k))
                q += 1
        groups.append(entries)
    return groups


def _ld_pairwise_args(plink, snps, indiv, window):
    if int(np.prod(plink.shape)) != snps * ((indiv + 3) // 4):
        raise ValueError(f"Matrix has wrong dimensions: {tuple(plink.shape)}")
    if not 0 <= int(window) < snps:
        raise ValueError(f"Window needs to be in [0, {snps}): {window}")


def ld_band_pairwise(plink, snps, indiv, window, kind="r"):
    """Additive (C entry mxa_ld_band_pairwise): ld_band() for PLINK data with missing genotypes -- the pairwise-complete r, Pearson's correlation over the
    individuals genotyped at both SNPs (NaN where there is none, or a SNP is constant on them).  Shape (snps, window + 1), out[i, d] = r(i, i + d)."""
    if kind not in ("r", "r2"):
        raise ValueError(f"kind needs to be 'r' or 'r2': {kind!r}")
    _ld_pairwise_args(plink, snps, indiv, window)
    L = _lib.check_library_handle()
    B = _zeros_like(plink, snps, int(window) + 1)
    _check(L.mxa_ld_band_pairwise(_lib.ptr(plink), int(snps), int(indiv), int(window), _lib.ptr(B), int(window) + 1, 1 if kind == "r2" else 0), "mxa_ld_band_pairwise")
    return B


def ld_scores_pairwise(plink, snps, indiv, window, adjust=False):
    """Additive (C entry mxa_ld_scores_pairwise): ld_scores() from the pairwise-complete r; adjust: r^2 - (1 - r^2) / (N_ij - 2) with the pair's own count of
    shared individuals.  Shape (snps,); fixed summation order (bitwise reproducible)."""
    _ld_pairwise_args(plink, snps, indiv, window)
    if adjust and indiv < 3:
        raise ValueError(f"The adjusted estimator needs at least 3 individuals: {indiv}")
    L = _lib.check_library_handle()
    S = _zeros_like(plink, snps)
    _check(L.mxa_ld_scores_pairwise(_lib.ptr(plink), int(snps), int(indiv), int(window), _lib.ptr(S), int(bool(adjust))), "mxa_ld_scores_pairwise")
    return S
