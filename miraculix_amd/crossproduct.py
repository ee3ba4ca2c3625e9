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
    """Tile rows per group of the pairwise entries (LdGroups in csrc/mxa_ldwindow.hip, the fixed window): as many as keep the count scratch (pairs slots of 256 KiB per band tile, a tile row holding up to
    min(nb, ceil(window / 256) + 1) tiles) under scratch_mb MiB -- one tile row at least, the whole band at most."""
    nb = (snps + 255) // 256
    row_tiles = min(nb, (window + 255) // 256 + 1)
    return max(1, min(nb, (scratch_mb << 20) // (row_tiles * pairs * PAIRWISE_SLOT_BYTES)))


def ld_pairwise_tiles(snps, window, group):
    """The tile plan of the pairwise entries (pairwise_group_tiles in csrc/mxa_ldwindow.hip), restated: the band tiles of ld_band_tiles in groups of `group` tile rows; per band tile (I, J) six entries
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


# ---- windowed LD by distance: C entries mxa_ld_window_bounds (host only) and mxa_ld_window_rows / _scores / _rows_pairwise / _scores_pairwise.
# The window of SNP i is [i, last[i]] (and, by symmetry, every k < i with last[k] >= i); last is non-decreasing with i <= last[i] < snps.
def ld_window_bounds(pos, chrom=None, max_dist=None, max_snps=None, snps=None):
    """Additive (C entry mxa_ld_window_bounds; no device needed): (last, rowptr) of a window by distance.  last[i] is the largest j >= i on i's chromosome
    with pos[j] - pos[i] <= max_dist and j - i <= max_snps; rowptr is the exclusive prefix sum of last[i] - i + 1 (int64, snps + 1 long).  pos: base pairs or
    centimorgans, non-decreasing inside a chromosome (None: no distance bound; then max_snps is required and `snps`, or chrom, gives the length); chrom: int
    codes, contiguous (None: one chromosome); max_snps None: no SNP bound."""
    if pos is not None:
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        n = len(pos)
        if max_dist is None:
            raise ValueError("max_dist is required with pos")
    else:
        n = len(chrom) if chrom is not None else snps
        if n is None:
            raise ValueError("without pos, snps (or chrom) gives the number of SNPs")
    if chrom is not None:
        chrom = np.ascontiguousarray(chrom, dtype=np.int32)
        if len(chrom) != n:
            raise ValueError(f"chrom needs one code per SNP: {len(chrom)} for {n}")
    L = _lib.check_library_handle()
    last = np.zeros(max(int(n), 0), dtype=np.int32)
    rowptr = np.zeros(max(int(n), 0) + 1, dtype=np.int64)
    _check(L.mxa_ld_window_bounds(int(n), _lib.ptr(pos), _lib.ptr(chrom), 0.0 if pos is None else float(max_dist), -1 if max_snps is None else int(max_snps),
                                  _lib.ptr(last), _lib.ptr(rowptr)), "mxa_ld_window_bounds")
    return last, rowptr


def ld_window_tiles(last):
    """The tile plan of the entries over `last`, restated: tile row I holds the tiles (I, J), I <= J <= jmax[I] = last[min(256 I + 255, snps - 1)] // 256 -- last
    is non-decreasing, so the tile row reaches as far as its last SNP does, and every listed tile holds a window element.  With last[i] = min(i + w, snps - 1)
    this is ld_band_tiles(snps, w)."""
    last = np.asarray(last)
    snps = len(last)
    nb = (snps + 255) // 256
    return [(i, j) for i in range(nb) for j in range(i, int(last[min(256 * i + 255, snps - 1)]) // 256 + 1)]


def _ld_last_args(plink, snps, indiv, last):
    """(last in the form the C entry takes, number of stored entries rowptr[snps]); the host copy is checked here, the library checks again"""
    if int(np.prod(plink.shape)) != snps * ((indiv + 3) // 4):
        raise ValueError(f"Matrix has wrong dimensions: {tuple(plink.shape)}")
    if _lib.is_torch_tensor(last):
        import torch
        if last.dtype != torch.int32 or last.numel() != snps:
            raise ValueError(f"last needs to be {snps} int32 values")
        h = last.cpu().numpy()
        last = last.contiguous()
    else:
        h = last = np.ascontiguousarray(last, dtype=np.int32)
        if last.shape != (snps,):
            raise ValueError(f"last needs to be {snps} int32 values")
    i = np.arange(snps)
    if np.any(h < i) or np.any(h >= snps) or np.any(np.diff(h) < 0):
        raise ValueError("last needs i <= last[i] < snps, non-decreasing")
    return last, int((h.astype(np.int64) - i + 1).sum())


def ld_window_rows(plink, snps, indiv, last, kind="r", is_plink_format=False, allele_freq=None):
    """Additive (C entry mxa_ld_window_rows): the entries R(i, i + d), 0 <= d <= last[i] - i, of ld()'s R as ragged rows: a flat array of rowptr[snps] values
    with out[rowptr[i] + d] = R(i, i + d) (rowptr as ld_window_bounds returns it).  No padding to the widest window.  kind "r" or "r2"."""
    if kind not in ("r", "r2"):
        raise ValueError(f"kind needs to be 'r' or 'r2': {kind!r}")
    if allele_freq is None or len(allele_freq) != snps:
        raise ValueError(f"Allele frequencies need to be equal to length of SNPs {snps}.")
    last, total = _ld_last_args(plink, snps, indiv, last)
    f = allele_freq if _lib.is_torch_tensor(allele_freq) else np.ascontiguousarray(allele_freq, dtype=np.float64)
    L = _lib.check_library_handle()
    B = _zeros_like(plink, total)
    _check(L.mxa_ld_window_rows(_lib.ptr(plink), int(snps), int(indiv), _lib.ptr(last), _lib.ptr(B), 1 if kind == "r2" else 0, int(bool(is_plink_format)), _lib.ptr(f)),
           "mxa_ld_window_rows")
    return B


def ld_window_scores(plink, snps, indiv, last, adjust=False, is_plink_format=False, allele_freq=None):
    """Additive (C entry mxa_ld_window_scores): ld_scores() over the window `last`: l_i = sum of t(r_ij) over first[i] <= j <= last[i], first[i] = the smallest k
    with last[k] >= i.  Shape (snps,); fixed summation order (bitwise reproducible)."""
    if allele_freq is None or len(allele_freq) != snps:
        raise ValueError(f"Allele frequencies need to be equal to length of SNPs {snps}.")
    if adjust and indiv < 3:
        raise ValueError(f"The adjusted estimator needs at least 3 individuals: {indiv}")
    last, _ = _ld_last_args(plink, snps, indiv, last)
    f = allele_freq if _lib.is_torch_tensor(allele_freq) else np.ascontiguousarray(allele_freq, dtype=np.float64)
    L = _lib.check_library_handle()
    S = _zeros_like(plink, snps)
    _check(L.mxa_ld_window_scores(_lib.ptr(plink), int(snps), int(indiv), _lib.ptr(last), _lib.ptr(S), int(bool(adjust)), int(bool(is_plink_format)), _lib.ptr(f)),
           "mxa_ld_window_scores")
    return S


def ld_window_rows_pairwise(plink, snps, indiv, last, kind="r"):
    """Additive (C entry mxa_ld_window_rows_pairwise): ld_window_rows() from the pairwise-complete r of ld_band_pairwise() (PLINK data with missing genotypes)."""
    if kind not in ("r", "r2"):
        raise ValueError(f"kind needs to be 'r' or 'r2': {kind!r}")
    last, total = _ld_last_args(plink, snps, indiv, last)
    L = _lib.check_library_handle()
    B = _zeros_like(plink, total)
    _check(L.mxa_ld_window_rows_pairwise(_lib.ptr(plink), int(snps), int(indiv), _lib.ptr(last), _lib.ptr(B), 1 if kind == "r2" else 0), "mxa_ld_window_rows_pairwise")
    return B


def ld_window_scores_pairwise(plink, snps, indiv, last, adjust=False):
    """Additive (C entry mxa_ld_window_scores_pairwise): ld_window_scores() from the pairwise-complete r, the adjustment with the pair's own N_ij."""
    if adjust and indiv < 3:
        raise ValueError(f"The adjusted estimator needs at least 3 individuals: {indiv}")
    last, _ = _ld_last_args(plink, snps, indiv, last)
    L = _lib.check_library_handle()
    S = _zeros_like(plink, snps)
    _check(L.mxa_ld_window_scores_pairwise(_lib.ptr(plink), int(snps), int(indiv), _lib.ptr(last), _lib.ptr(S), int(bool(adjust))), "mxa_ld_window_scores_pairwise")
    return S


# ---- the pairs of a window above an r^2 cutoff as CSR: C entries mxa_ld_window_pairs / mxa_ld_window_pairs_pairwise
def ld_pairs(plink, snps, indiv, last=None, window=None, min_r2=0.2, kind="r2", pairwise=False, is_plink_format=False, allele_freq=None, capacity=None):
    """Additive (C entries mxa_ld_window_pairs, mxa_ld_window_pairs_pairwise): the pairs i < j <= last[i] with r^2 >= min_r2 as CSR of the strict upper
    triangle, compacted on the device -- what PLINK's --r2 --ld-window-kb .. --ld-window-r2 lists.  Returns (rowptr int64 of snps + 1, col int32, val float64),
    numpy or torch tensors on the input's device: the kept pairs of SNP i are col[rowptr[i]: rowptr[i + 1]] (ascending) with val = r (kind "r") or r * r
    (kind "r2"); r is the value ld_window_rows() / ld_window_rows_pairwise() (pairwise=True: data with missing genotypes) stores for the pair, bit for bit.
    Exactly one of `last` (as ld_window_bounds returns it) and `window` (a fixed number of SNPs: last[i] = min(i + window, snps - 1)) is given.
    capacity=None: a count-only call, then an exactly sized filling call -- the tile products run twice.  capacity=k: one call into arrays of k entries,
    trimmed to the total; raises RuntimeError naming the needed total when it exceeds k."""
    if kind not in ("r", "r2"):
        raise ValueError(f"kind needs to be 'r' or 'r2': {kind!r}")
    if (last is None) == (window is None):
        raise ValueError("exactly one of last and window is needed")
    if not pairwise and (allele_freq is None or len(allele_freq) != snps):
        raise ValueError(f"Allele frequencies need to be equal to length of SNPs {snps}.")
    if window is not None:
        if not 0 <= int(window) < snps:
            raise ValueError(f"Window needs to be in [0, {snps}): {window}")
        last = np.minimum(np.arange(snps, dtype=np.int64) + int(window), snps - 1).astype(np.int32)
    last, _ = _ld_last_args(plink, snps, indiv, last)
    import ctypes
    L = _lib.check_library_handle()
    if _lib.is_torch_tensor(plink):
        import torch
        new = lambda n, dt: torch.zeros(n, dtype={np.int64: torch.int64, np.int32: torch.int32, np.float64: torch.float64}[dt], device=plink.device)
    else:
        new = lambda n, dt: np.zeros(n, dtype=dt)
    entry = "mxa_ld_window_pairs_pairwise" if pairwise else "mxa_ld_window_pairs"
    tail = []
    if not pairwise:
        f = allele_freq if _lib.is_torch_tensor(allele_freq) else np.ascontiguousarray(allele_freq, dtype=np.float64)
        tail = [int(bool(is_plink_format)), _lib.ptr(f)]
    rowptr = new(snps + 1, np.int64)
    total = ctypes.c_long(0)

    def call(col, val, cap):
        return getattr(L, entry)(_lib.ptr(plink), int(snps), int(indiv), _lib.ptr(last), float(min_r2), 1 if kind == "r2" else 0, _lib.ptr(rowptr), _lib.ptr(col),
                                 _lib.ptr(val), int(cap), ctypes.byref(total), *tail)

    if capacity is None:
        _check(call(None, None, 0), entry)
        capacity = total.value
    elif int(capacity) < 0:
        raise ValueError(f"capacity must not be negative: {capacity}")
    col, val = new(int(capacity), np.int32), new(int(capacity), np.float64)
    _check(call(col, val, int(capacity)), entry)               # error 25: the message names the total and the capacity
    return rowptr, col[: total.value], val[: total.value]


# ---- the window applied to a matrix, Y = T_w(R) X: C entries mxa_ld_window_apply / mxa_ld_window_apply_pairwise
LD_APPLY_TERMS = {"r": 0, "r2": 1, "r2_adj": 2}
LD_APPLY_NC = 16                                              # columns of X per workgroup of the tile kernel (kLdApplyNC)


def ld_window_apply(plink, snps, indiv, X, last=None, window=None, term="r2", pairwise=False, is_plink_format=False, allele_freq=None, out=None):
    """Additive (C entries mxa_ld_window_apply, mxa_ld_window_apply_pairwise): Y = T_w(R) X, Y[i, c] = sum over the window of SNP i (first[i] <= j <= last[i],
    both sides of i) of t(r_ij) X[j, c], without writing the window's rows.  X: (snps, n) or (snps,) float64, numpy or a torch tensor (host / device); the
    result has X's shape and kind.  term "r" (t = r: R_w X), "r2" (partitioned LD scores) or "r2_adj" (the adjusted term of the scores entries).  Exactly one of
    `last` and `window`, as for ld_pairs().  Every sum runs in a fixed order: the same bits for every engine, pointer kind, scratch size and n.  A monomorphic
    SNP makes every row whose window holds it NaN: filter first.  out: a (snps, n) result to fill, Fortran-ordered numpy or a torch tensor whose transpose is
    contiguous (n rows of snps values)."""
    if term not in LD_APPLY_TERMS:
        raise ValueError(f"term needs to be 'r', 'r2' or 'r2_adj': {term!r}")
    if (last is None) == (window is None):
        raise ValueError("exactly one of last and window is needed")
    if not pairwise and (allele_freq is None or len(allele_freq) != snps):
        raise ValueError(f"Allele frequencies need to be equal to length of SNPs {snps}.")
    if term == "r2_adj" and indiv < 3:
        raise ValueError(f"The adjusted estimator needs at least 3 individuals: {indiv}")
    shape = tuple(X.shape)
    if len(shape) not in (1, 2) or shape[0] != snps or (len(shape) == 2 and shape[1] < 1):
        raise ValueError(f"X needs to be ({snps},) or ({snps}, n >= 1): {shape}")
    n = 1 if len(shape) == 1 else int(shape[1])
    if window is not None:
        if not 0 <= int(window) < snps:
            raise ValueError(f"Window needs to be in [0, {snps}): {window}")
        last = np.minimum(np.arange(snps, dtype=np.int64) + int(window), snps - 1).astype(np.int32)
    last, _ = _ld_last_args(plink, snps, indiv, last)
    # column-major operands: n contiguous columns of snps values
    if _lib.is_torch_tensor(X):
        import torch
        if X.dtype != torch.float64:
            raise ValueError("X needs to be float64")
        xc = X.reshape(snps, n).t().contiguous()              # (n, snps) row-major = (snps, n) column-major
        yc = torch.zeros((n, snps), dtype=torch.float64, device=X.device) if out is None else out.t()
        if out is not None and (tuple(out.shape) != (snps, n) or out.dtype != torch.float64 or not yc.is_contiguous()):
            raise ValueError(f"out needs to be a float64 ({snps}, {n}) tensor with contiguous columns")
    else:
        xc = np.ascontiguousarray(np.asarray(X, dtype=np.float64).reshape(snps, n).T)
        yc = np.zeros((n, snps), dtype=np.float64) if out is None else out.T
        if out is not None and (out.shape != (snps, n) or out.dtype != np.float64 or not yc.flags.c_contiguous):
            raise ValueError(f"out needs to be a float64 ({snps}, {n}) array in Fortran order")
    L = _lib.check_library_handle()
    head = [_lib.ptr(plink), int(snps), int(indiv), _lib.ptr(last), LD_APPLY_TERMS[term], _lib.ptr(xc), int(snps), n, _lib.ptr(yc), int(snps)]
    if pairwise:
        _check(L.mxa_ld_window_apply_pairwise(*head), "mxa_ld_window_apply_pairwise")
    else:
        f = allele_freq if _lib.is_torch_tensor(allele_freq) else np.ascontiguousarray(allele_freq, dtype=np.float64)
        _check(L.mxa_ld_window_apply(*head, int(bool(is_plink_format)), _lib.ptr(f)), "mxa_ld_window_apply")
    if out is not None:
        return out
    Y = yc.t() if _lib.is_torch_tensor(yc) else yc.T
    return Y.reshape(shape)


def ld_scores_partitioned(plink, snps, indiv, annot, last=None, window=None, adjust=False, pairwise=False, is_plink_format=False, allele_freq=None):
    """Partitioned (stratified) LD scores l(i, c) = sum over the window of SNP i of t(r_ij) annot[j, c] (ldsc --l2 --annot; the input of S-LDSC): annot is
    (snps, n) -- a base column of ones gives ld_window_scores() up to the order of the sums.  adjust: the adjusted term.  A wrapper of ld_window_apply()."""
    return ld_window_apply(plink, snps, indiv, annot, last=last, window=window, term="r2_adj" if adjust else "r2", pairwise=pairwise,
                           is_plink_format=is_plink_format, allele_freq=allele_freq)


# ---- LD pruning / clumping, the greedy selection on the pairs graph: C entries mxa_ld_window_prune / mxa_ld_window_prune_pairwise / mxa_ld_prune_csr
def _prune_priority(priority, snps):
    """priority as the C entries take it (None, float64 numpy, or a contiguous float64 tensor); NaN is refused here, the library checks again"""
    if priority is None:
        return None
    if _lib.is_torch_tensor(priority):
        import torch
        if priority.dtype != torch.float64 or priority.numel() != snps:
            raise ValueError(f"priority needs to be {snps} float64 values")
        if bool(torch.isnan(priority).any()):
            raise ValueError("priority must not hold a NaN")
        return priority.contiguous()
    priority = np.ascontiguousarray(priority, dtype=np.float64)
    if priority.shape != (snps,):
        raise ValueError(f"priority needs to be {snps} float64 values")
    if np.isnan(priority).any():
        raise ValueError("priority must not hold a NaN")
    return priority


def _prune_call(like, snps, return_owner, return_rounds, entry, call):
    """keep / owner next to `like` (numpy, or torch on like's device), the call, and the results in the order (keep[, owner][, rounds])"""
    import ctypes
    if _lib.is_torch_tensor(like):
        import torch
        keep = torch.zeros(snps, dtype=torch.uint8, device=like.device)
        owner = torch.zeros(snps, dtype=torch.int32, device=like.device) if return_owner else None
    else:
        keep = np.zeros(snps, dtype=np.uint8)
        owner = np.zeros(snps, dtype=np.int32) if return_owner else None
    n_kept, rounds = ctypes.c_long(0), ctypes.c_int(0)
    _check(call(_lib.ptr(keep), _lib.ptr(owner), ctypes.byref(n_kept), ctypes.byref(rounds)), entry)
    keep = keep.bool() if _lib.is_torch_tensor(keep) else keep.astype(bool)
    out = (keep,) + ((owner,) if return_owner else ()) + ((rounds.value,) if return_rounds else ())
    return out[0] if len(out) == 1 else out


def ld_prune(plink, snps, indiv, last=None, window=None, min_r2=0.2, priority=None, pairwise=False, is_plink_format=False, allele_freq=None, return_owner=False,
             return_rounds=False):
    """Additive (C entries mxa_ld_window_prune, mxa_ld_window_prune_pairwise): LD pruning / clumping on the device.  The graph: the pairs ld_pairs() lists for
    the same plink, last | window, min_r2 and route.  The order: smaller priority first, ties by index (priority=None: index order) -- p-values for clumping,
    -MAF for pruning.  The result: walk the SNPs in that order, keep a SNP iff none of its neighbours has been kept (unique: the same on every engine).
    Returns keep (bool, snps), or (keep, owner) with return_owner: owner[v] = v for a kept SNP, else the kept neighbour that removed it (int32; PLINK's index
    SNP of the clump); return_rounds appends the number of rounds the device ran (the longest dependency chain).  numpy, or torch tensors on plink's device.
    Exactly one of `last` and `window` is given, as for ld_pairs().  The pair list stays on the device; the window's products run twice (count, fill)."""
    if (last is None) == (window is None):
        raise ValueError("exactly one of last and window is needed")
    if not pairwise and (allele_freq is None or len(allele_freq) != snps):
        raise ValueError(f"Allele frequencies need to be equal to length of SNPs {snps}.")
    if window is not None:
        if not 0 <= int(window) < snps:
            raise ValueError(f"Window needs to be in [0, {snps}): {window}")
        last = np.minimum(np.arange(snps, dtype=np.int64) + int(window), snps - 1).astype(np.int32)
    last, _ = _ld_last_args(plink, snps, indiv, last)
    priority = _prune_priority(priority, snps)
    L = _lib.check_library_handle()
    entry = "mxa_ld_window_prune_pairwise" if pairwise else "mxa_ld_window_prune"
    tail = []
    if not pairwise:
        f = allele_freq if _lib.is_torch_tensor(allele_freq) else np.ascontiguousarray(allele_freq, dtype=np.float64)
        tail = [int(bool(is_plink_format)), _lib.ptr(f)]
    return _prune_call(plink, snps, return_owner, return_rounds, entry, lambda keep, owner, n_kept, rounds: getattr(L, entry)(
        _lib.ptr(plink), int(snps), int(indiv), _lib.ptr(last), float(min_r2), _lib.ptr(priority), keep, owner, n_kept, rounds, *tail))


def ld_prune_csr(rowptr, col, priority=None, return_owner=False, return_rounds=False):
    """Additive (C entry mxa_ld_prune_csr): the graph step of ld_prune() alone, on a CSR of the strict upper triangle such as ld_pairs() returns (rowptr int64
    of snps + 1, col int32, ascending in a row) -- one pair list pruned under several priorities without repeating the products.  Results as ld_prune(), next
    to rowptr (numpy, or torch on rowptr's device)."""
    def arr(a, np_dt, what):
        if _lib.is_torch_tensor(a):
            import torch
            if a.dtype != {np.int64: torch.int64, np.int32: torch.int32}[np_dt]:
                raise ValueError(f"{what} needs to be {np.dtype(np_dt).name}")
            return a.contiguous()
        return np.ascontiguousarray(a, dtype=np_dt)
    rowptr, col = arr(rowptr, np.int64, "rowptr"), arr(col, np.int32, "col")
    snps = int(np.prod(rowptr.shape)) - 1
    if snps < 1:
        raise ValueError("rowptr needs snps + 1 >= 2 entries")
    priority = _prune_priority(priority, snps)
    L = _lib.check_library_handle()
    return _prune_call(rowptr, snps, return_owner, return_rounds, "mxa_ld_prune_csr", lambda keep, owner, n_kept, rounds: L.mxa_ld_prune_csr(
        int(snps), _lib.ptr(rowptr), _lib.ptr(col) if int(np.prod(col.shape)) else None, _lib.ptr(priority), keep, owner, n_kept, rounds))


# ---- the LD operator object: the window's values staged once on the device, then applied and ridge-solved there (C entries mxa_ld_op_*)
LD_OP_KINDS = {"r": 0, "r2": 1}
LD_OP_STATUS = ("converged", "max_iter reached", "breakdown")


def _host_last(last, snps):
    """`last` as a checked int32 numpy array of snps values"""
    if _lib.is_torch_tensor(last):
        last = last.cpu().numpy()
    last = np.ascontiguousarray(last, dtype=np.int32)
    if last.shape != (snps,):
        raise ValueError(f"last needs to be {snps} int32 values")
    i = np.arange(snps)
    if np.any(last < i) or np.any(last >= snps) or np.any(np.diff(last) < 0):
        raise ValueError("last needs i <= last[i] < snps, non-decreasing")
    return last


def ld_op_bytes(last):
    """Additive (C entry mxa_ld_op_bytes; no device needed): (entries, bytes) of the LdOperator of the window `last` -- the number of upper ragged entries
    rowptr[snps], and the device bytes the object holds after creation (the mirrored rows, 2 entries - snps doubles, and its index arrays).  During
    creation the upper rows (8 entries bytes) stand next to it."""
    import ctypes
    snps = int(np.prod(np.shape(last)))
    if snps < 1:
        raise ValueError("last needs at least one value")
    last = _host_last(last, snps)
    entries, nbytes = ctypes.c_long(0), ctypes.c_long(0)
    _check(_lib.check_library_handle().mxa_ld_op_bytes(snps, _lib.ptr(last), ctypes.byref(entries), ctypes.byref(nbytes)), "mxa_ld_op_bytes")
    return entries.value, nbytes.value


def _window_or_last(snps, last, window):
    if (last is None) == (window is None):
        raise ValueError("exactly one of last and window is needed")
    if window is not None:
        if not 0 <= int(window) < snps:
            raise ValueError(f"Window needs to be in [0, {snps}): {window}")
        last = np.minimum(np.arange(snps, dtype=np.int64) + int(window), snps - 1).astype(np.int32)
    return last


class LdOperator:
    """The windowed LD matrix T_w(R) (kind "r") or its element-wise square (kind "r2") resident on the device: created once, then applied
    (Y = shift X + T X) and ridge-solved ((T + shift I) X = B, conjugate gradients) any number of times without repeating the genotype products.
    T is bit for bit what ld_window_rows / ld_window_rows_pairwise return.  Use as a context manager, or call free()."""

    def __init__(self, handle, snps, last):
        self._h = handle
        self.snps = snps
        self.last = last
        self.entries, self.nbytes = ld_op_bytes(last)

    @classmethod
    def create(cls, plink, snps, indiv, last=None, window=None, kind="r", pairwise=False, is_plink_format=False, allele_freq=None):
        """from the packed genotypes: arguments as ld_window_rows / ld_window_rows_pairwise; exactly one of `last` and `window`"""
        import ctypes
        if kind not in LD_OP_KINDS:
            raise ValueError(f"kind needs to be 'r' or 'r2': {kind!r}")
        if not pairwise and (allele_freq is None or len(allele_freq) != snps):
            raise ValueError(f"Allele frequencies need to be equal to length of SNPs {snps}.")
        last = _window_or_last(snps, last, window)
        host = _host_last(last, snps)
        last, _ = _ld_last_args(plink, snps, indiv, last)
        L = _lib.check_library_handle()
        h = ctypes.c_void_p(None)
        if pairwise:
            _check(L.mxa_ld_op_create_pairwise(_lib.ptr(plink), int(snps), int(indiv), _lib.ptr(last), LD_OP_KINDS[kind], ctypes.byref(h)), "mxa_ld_op_create_pairwise")
        else:
            f = allele_freq if _lib.is_torch_tensor(allele_freq) else np.ascontiguousarray(allele_freq, dtype=np.float64)
            _check(L.mxa_ld_op_create(_lib.ptr(plink), int(snps), int(indiv), _lib.ptr(last), LD_OP_KINDS[kind], int(bool(is_plink_format)), _lib.ptr(f),
                                      ctypes.byref(h)), "mxa_ld_op_create")
        return cls(h, int(snps), host)

    @classmethod
    def from_rows(cls, last, rows):
        """from upper ragged rows (ld_window_rows' layout: rows[rowptr[i] + d] = T(i, i + d)), numpy or a torch tensor (host / device); copied"""
        import ctypes
        snps = int(np.prod(np.shape(last)))
        if snps < 1:
            raise ValueError("last needs at least one value")
        host = _host_last(last, snps)
        total = int((host.astype(np.int64) - np.arange(snps) + 1).sum())
        if _lib.is_torch_tensor(rows):
            import torch
            if rows.dtype != torch.float64 or rows.numel() != total:
                raise ValueError(f"rows needs to be {total} float64 values")
            rows = rows.contiguous()
        else:
            rows = np.ascontiguousarray(rows, dtype=np.float64)
            if rows.shape != (total,):
                raise ValueError(f"rows needs to be {total} float64 values")
        h = ctypes.c_void_p(None)
        _check(_lib.check_library_handle().mxa_ld_op_from_rows(snps, _lib.ptr(host), _lib.ptr(rows), ctypes.byref(h)), "mxa_ld_op_from_rows")
        return cls(h, snps, host)

    def _live(self):
        if self._h is None or not self._h.value:
            raise RuntimeError("the LdOperator has been freed")
        return _lib.check_library_handle()

    def _columns(self, X, what):
        """(column-major copy of X as n rows of snps values, n, X's shape)"""
        shape = tuple(X.shape)
        if len(shape) not in (1, 2) or shape[0] != self.snps or (len(shape) == 2 and shape[1] < 1):
            raise ValueError(f"{what} needs to be ({self.snps},) or ({self.snps}, n >= 1): {shape}")
        n = 1 if len(shape) == 1 else int(shape[1])
        if _lib.is_torch_tensor(X):
            import torch
            if X.dtype != torch.float64:
                raise ValueError(f"{what} needs to be float64")
            return X.reshape(self.snps, n).t().contiguous(), n, shape
        return np.ascontiguousarray(np.asarray(X, dtype=np.float64).reshape(self.snps, n).T), n, shape

    def _result(self, like, n, out):
        snps = self.snps
        if _lib.is_torch_tensor(like):
            import torch
            yc = torch.zeros((n, snps), dtype=torch.float64, device=like.device) if out is None else out.t()
            if out is not None and (tuple(out.shape) != (snps, n) or out.dtype != torch.float64 or not yc.is_contiguous()):
                raise ValueError(f"out needs to be a float64 ({snps}, {n}) tensor with contiguous columns")
        else:
            yc = np.zeros((n, snps), dtype=np.float64) if out is None else out.T
            if out is not None and (out.shape != (snps, n) or out.dtype != np.float64 or not yc.flags.c_contiguous):
                raise ValueError(f"out needs to be a float64 ({snps}, {n}) array in Fortran order")
        return yc

    def apply(self, X, shift=0.0, out=None):
        """Y = shift X + T X.  X: (snps, n) or (snps,) float64, numpy or torch (host / device); the result has X's shape and kind.  The same bits from run
        to run, for host and device operands and for every n.  out: as for ld_window_apply()."""
        L = self._live()
        if not np.isfinite(shift):
            raise ValueError(f"shift needs to be finite: {shift}")
        xc, n, shape = self._columns(X, "X")
        yc = self._result(xc, n, out)
        _check(L.mxa_ld_op_apply(self._h, float(shift), _lib.ptr(xc), self.snps, n, _lib.ptr(yc), self.snps), "mxa_ld_op_apply")
        if out is not None:
            return out
        return (yc.t() if _lib.is_torch_tensor(yc) else yc.T).reshape(shape)

    def solve(self, B, shift, tol=1e-8, max_iter=1000):
        """(T + shift I) X = B by conjugate gradients from X = 0, every column on its own.  Returns (X, iters, relres, status): X of B's shape and kind; iters
        (int32), relres (the final recurrence residual over |b|) and status (0 converged, 1 max_iter reached, 2 breakdown: not positive definite, or a NaN) as
        numpy arrays of n."""
        L = self._live()
        if not np.isfinite(shift):
            raise ValueError(f"shift needs to be finite: {shift}")
        if not 0.0 < tol < 1.0:
            raise ValueError(f"tol needs to be in (0, 1): {tol}")
        if int(max_iter) < 0:
            raise ValueError(f"max_iter must not be negative: {max_iter}")
        bc, n, shape = self._columns(B, "B")
        xc = self._result(bc, n, None)
        iters, relres, status = np.zeros(n, np.int32), np.zeros(n, np.float64), np.zeros(n, np.int32)
        _check(L.mxa_ld_op_solve(self._h, float(shift), _lib.ptr(bc), self.snps, n, _lib.ptr(xc), self.snps, float(tol), int(max_iter), _lib.ptr(iters),
                                 _lib.ptr(relres), _lib.ptr(status)), "mxa_ld_op_solve")
        return (xc.t() if _lib.is_torch_tensor(xc) else xc.T).reshape(shape), iters, relres, status

    def rows(self, like=None):
        """the upper ragged rows (ld_window_rows' layout) as a numpy array, or as a torch tensor next to `like`"""
        L = self._live()
        out = _zeros_like(like if like is not None else self.last, self.entries)
        _check(L.mxa_ld_op_rows(self._h, _lib.ptr(out)), "mxa_ld_op_rows")
        return out

    def free(self):
        if self._h is not None and self._h.value:
            import ctypes
            _lib.check_library_handle().mxa_ld_op_free(ctypes.byref(self._h))
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
