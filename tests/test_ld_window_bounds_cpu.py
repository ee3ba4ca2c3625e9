"""Windows by distance, the host side (no device): mxa_ld_window_bounds against its O(n^2) definition in numpy -- last[i] = the largest j >= i with
chrom[j] == chrom[i], pos[j] - pos[i] <= max_dist (one rounded fp64 subtraction, inclusive) and j - i <= max_snps; rowptr = the exclusive prefix sum of
last[i] - i + 1 -- on seeded inputs with tied positions, gaps above max_dist, one-SNP chromosomes and chromosome ends at the indices 255, 256 and 257,
with the SNP bound alone and with both bounds; every argument error returns 1 and leaves the outputs alone.  And the tile plan over `last`, restated in
miraculix_amd.crossproduct.ld_window_tiles: every window element lies in exactly one listed tile, no listed tile is without one, and for
last[i] = min(i + w, snps - 1) the list is ld_band_tiles(snps, w)."""
import ctypes

import numpy as np
import pytest

from miraculix_amd import lib as mxlib
from miraculix_amd.crossproduct import ld_band_tiles, ld_window_bounds, ld_window_tiles

T = 256
SENT_I, SENT_L = -7, -9


def _definition(pos, chrom, max_dist, max_snps):
    """the O(n^2) definition: per i the largest j >= i for which all given bounds hold"""
    n = len(pos) if pos is not None else len(chrom)
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    ok = j >= i
    if chrom is not None:
        ok &= chrom[None, :] == chrom[:, None]
    if pos is not None:
        ok &= (pos[None, :] - pos[:, None]) <= max_dist
    if max_snps is not None:
        ok &= (j - i) <= max_snps
    last = np.where(ok, j, -1).max(axis=1)
    rowptr = np.concatenate([[0], np.cumsum(last - np.arange(n) + 1)])
    return last.astype(np.int32), rowptr.astype(np.int64)


def _genome(seed, lengths, max_dist, tie_frac=0.2, big_gap_frac=0.05):
    """positions per chromosome: cumulative seeded gaps, a share of them 0 (ties) and a share above max_dist; every chromosome starts again near 0"""
    rng = np.random.default_rng(seed)
    pos, chrom = [], []
    for c, ln in enumerate(lengths):
        gaps = rng.exponential(max_dist / 40.0, size=ln)
        gaps[rng.random(ln) < tie_frac] = 0.0
        gaps[rng.random(ln) < big_gap_frac] = max_dist * (1.0 + rng.random())
        pos.append(np.cumsum(gaps) + rng.random())
        chrom.append(np.full(ln, 3 * c + 1))         # codes need not be consecutive
    return np.concatenate(pos), np.concatenate(chrom).astype(np.int32)


# chromosome ends at 255, 256, 257 (the tile edge), one-SNP chromosomes, a long rest
CASES = [
    ("edges", [255, 1, 1, 254, 1, 700, 788], 1.0),      # ends at 255, 256, 257, 511, 512, 1212, 2000
    ("short", [1, 1, 1], 5.0),
    ("one", [1], 1.0),
    ("single-chromosome", [1500], 250.0),
    ("many", [3, 1, 40, 1, 1, 200, 256, 257, 255, 13], 1e4),
]


@pytest.mark.parametrize("name,lengths,max_dist", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("bounds", ["dist", "snps", "both", "dist-no-chrom"])
def test_bounds_equal_the_quadratic_definition(name, lengths, max_dist, bounds):
    pos, chrom = _genome(len(lengths) * 7 + sum(lengths), lengths, max_dist)
    n = len(pos)
    assert n <= 2000
    if bounds == "dist-no-chrom":
        pos, chrom_arg = np.sort(pos), None                      # one chromosome: positions must not decrease
    else:
        chrom_arg = chrom
    ends = np.flatnonzero(np.diff(chrom)) + 1
    if name == "edges":
        assert {255, 256, 257} <= set(ends.tolist())
        assert np.any(np.diff(pos)[np.diff(chrom) == 0] == 0.0) and np.any(np.diff(pos)[np.diff(chrom) == 0] > max_dist)      # ties and gaps above max_dist
    for max_snps in ((0, 1, 37, 300) if bounds in ("snps", "both") else (None,)):
        p = None if bounds == "snps" else pos
        want_last, want_rowptr = _definition(p, chrom_arg, max_dist, max_snps)
        last, rowptr = ld_window_bounds(p, chrom_arg, max_dist=None if p is None else max_dist, max_snps=max_snps, snps=n)
        assert last.dtype == np.int32 and rowptr.dtype == np.int64
        assert np.array_equal(last, want_last), (name, bounds, max_snps)
        assert np.all(np.diff(last) >= 0) and np.all(last >= np.arange(n)) and np.all(last < n)
        assert np.array_equal(rowptr, want_rowptr), (name, bounds, max_snps)
        assert rowptr[-1] == int((last.astype(np.int64) - np.arange(n) + 1).sum())


def test_rowptr_is_optional_and_the_comparison_is_inclusive():
    L = mxlib.check_library_handle()
    pos = np.array([0.0, 0.1, 0.1 + 0.2, 0.7, 1.0])               # 0.1 + 0.2 - 0.0 > 0.3 in fp64: the comparison sees the rounded difference
    last = np.full(5, SENT_I, dtype=np.int32)
    assert L.mxa_ld_window_bounds(5, mxlib.ptr(pos), None, ctypes.c_double(0.3), -1, mxlib.ptr(last), None) == 0
    want, _ = _definition(pos, None, 0.3, None)
    assert np.array_equal(last, want) and last[0] == 1
    assert L.mxa_ld_window_bounds(5, mxlib.ptr(pos), None, ctypes.c_double(0.7), -1, mxlib.ptr(last), None) == 0
    assert last[0] == 3                                           # 0.7 - 0.0 <= 0.7: inclusive
    assert L.mxa_ld_window_bounds(5, mxlib.ptr(pos), None, ctypes.c_double(0.0), -1, mxlib.ptr(last), None) == 0
    assert np.array_equal(last, np.arange(5))


def test_every_argument_error_returns_one_and_leaves_the_outputs_alone():
    L = mxlib.check_library_handle()
    n = 6
    pos = np.array([1.0, 2.0, 3.0, 1.0, 2.0, 3.0])
    chrom = np.array([1, 1, 1, 2, 2, 2], dtype=np.int32)

    def call(snps=n, pos=pos, chrom=chrom, max_dist=1.0, max_snps=-1, with_last=True):
        last, rowptr = np.full(n, SENT_I, dtype=np.int32), np.full(n + 1, SENT_L, dtype=np.int64)
        rc = L.mxa_ld_window_bounds(snps, mxlib.ptr(pos), mxlib.ptr(chrom), ctypes.c_double(max_dist), max_snps, mxlib.ptr(last) if with_last else None, mxlib.ptr(rowptr))
        return rc, L.mxa_last_error(), bool(np.all(last == SENT_I) and np.all(rowptr == SENT_L))

    bad = (1, 1, True)
    assert call(snps=0) == bad and call(snps=-3) == bad
    assert call(with_last=False) == bad
    assert call(max_dist=-1.0) == bad
    assert call(max_dist=float("nan")) == bad
    assert call(pos=np.array([1.0, np.nan, 3.0, 1.0, 2.0, 3.0])) == bad
    assert call(pos=np.array([1.0, 3.0, 2.0, 1.0, 2.0, 3.0])) == bad             # decreases inside a chromosome
    assert call(chrom=None) == bad                                                # the same positions as one chromosome: 3.0 -> 1.0 decreases
    assert call(chrom=np.array([1, 1, 2, 2, 1, 1], dtype=np.int32)) == bad        # chromosome 1 returns
    assert call(pos=None, max_snps=-1) == bad                                     # neither bound
    # a position may decrease where the chromosome changes, and the next good call succeeds
    assert call() == (0, 0, False)
    assert call(pos=None, max_snps=2) == (0, 0, False)
    with pytest.raises(RuntimeError):
        ld_window_bounds(pos, np.array([1, 1, 2, 2, 1, 1]), max_dist=1.0)
    with pytest.raises(ValueError):
        ld_window_bounds(None, None, max_snps=3)


# ---------------------------------------------------------------------------------------------------------------------------- the tile plan
def _check_plan(last):
    n = len(last)
    nb = -(-n // T)
    tiles = ld_window_tiles(last)
    assert len(set(tiles)) == len(tiles)
    listed = np.zeros((nb, nb), dtype=np.int64)
    for ti, tj in tiles:
        assert 0 <= ti <= tj < nb
        listed[ti, tj] += 1
    reach = last.astype(np.int64) - np.arange(n)
    ii = np.repeat(np.arange(n), reach + 1)
    jj = ii + (np.arange(len(ii)) - np.repeat(np.cumsum(reach + 1) - (reach + 1), reach + 1))
    assert np.all(jj <= last[ii]) and len(ii) == int((reach + 1).sum())
    assert np.all(listed[ii // T, jj // T] == 1)                 # every window element in exactly one listed tile
    hit = np.zeros((nb, nb), dtype=bool)
    hit[ii // T, jj // T] = True
    assert np.array_equal(hit, listed == 1)                       # no listed tile without a window element
    return tiles


@pytest.mark.parametrize("name,lengths,max_dist", CASES, ids=[c[0] for c in CASES])
def test_window_plan_covers_the_window_exactly_once_and_nothing_else(name, lengths, max_dist):
    pos, chrom = _genome(11 + sum(lengths), lengths, max_dist, tie_frac=0.5)
    for md in (max_dist, 30 * max_dist):
        last, _ = ld_window_bounds(pos, chrom, max_dist=md)
        _check_plan(last)
        last, _ = ld_window_bounds(np.sort(pos), None, max_dist=md)
        _check_plan(last)


def test_window_plan_with_tile_rows_of_different_lengths():
    """600 SNPs at one position from index 200 on: reach 599 at SNP 200, 0 at the isolated SNPs around them"""
    n = 2000
    pos = np.arange(n, dtype=np.float64) * 10.0
    pos[200:800] = pos[200]
    last, _ = ld_window_bounds(pos, None, max_dist=1.0)
    reach = last - np.arange(n)
    assert reach.min() == 0 and reach.max() == 599
    tiles = _check_plan(last)
    per_row = np.bincount([t[0] for t in tiles], minlength=8)
    assert per_row.tolist() == [4, 3, 2, 1, 1, 1, 1, 1]


@pytest.mark.parametrize("snps,window", [(s, w) for s in (1, 130, 255, 256, 257, 777, 3000, 5000)
                                         for w in (0, 1, 254, 255, 256, 257, 511, 512, 513, 700, 4999) if w < s])    # the grid of test_ld_band_plan_cpu.py
def test_window_plan_of_a_fixed_window_is_the_band_plan(snps, window):
    last = np.minimum(np.arange(snps) + window, snps - 1).astype(np.int32)
    got, _ = ld_window_bounds(None, None, max_snps=window, snps=snps)
    assert np.array_equal(got, last)
    assert ld_window_tiles(last) == ld_band_tiles(snps, window)


# ------------------------------------------------------------------------------------------------------------------------------ the .bim map
def test_read_bim_gives_consecutive_chromosome_codes_centimorgans_and_base_pairs(tmp_path):
    from miraculix_amd.read_plink import read_bim
    lines = ["1 rs1 0.0 1000 A G", "1\trs2\t0.5\t2000\tA\tG", "1 rs3 0.5 2000 C T", "X rs4 0.1 500 A C", "chr2 rs5 1.25 700 G T", "chr2 rs6 3 900000 G T"]
    (tmp_path / "d.bim").write_text("\n".join(lines) + "\n")
    for path in (str(tmp_path / "d.bed"), str(tmp_path / "d.bim"), str(tmp_path / "d")):
        chrom, cm, bp = read_bim(path)
        assert chrom.dtype == np.int32 and chrom.tolist() == [0, 0, 0, 1, 2, 2]
        assert cm.tolist() == [0.0, 0.5, 0.5, 0.1, 1.25, 3.0] and bp.tolist() == [1000.0, 2000.0, 2000.0, 500.0, 700.0, 900000.0]
    last, rowptr = ld_window_bounds(cm, chrom, max_dist=1.0)
    assert last.tolist() == [2, 2, 2, 3, 4, 5] and rowptr.tolist() == [0, 3, 5, 6, 7, 8, 9]
    last, _ = ld_window_bounds(bp, chrom, max_dist=1000.0)
    assert last.tolist() == [2, 2, 2, 3, 4, 5]
    (tmp_path / "bad.bim").write_text("1 rs1 0.0 1000 A\n")
    with pytest.raises(ValueError):
        read_bim(str(tmp_path / "bad"))
