"""The tile plan of the windowed LD entries (mxa_ld_band, mxa_ld_scores), restated in miraculix_amd.crossproduct.ld_band_tiles: the 256 x 256 tiles
(I, J), I <= J <= I + ceil(window / 256).  Checked against the definition of the band itself, element by element: the number of tiles is the count
derived from (snps, window), every (i, j) with 0 <= j - i <= window lies in exactly one listed tile, and no listed tile lies wholly outside the band.
(The library's planner is the same two loops in C++; the GPU tests check its results element by element against mxa_ld.)"""
import numpy as np
import pytest

from miraculix_amd.crossproduct import ld_band_tiles

T = 256


def _derived_count(snps, window):
    """tile diagonal dt holds nb - dt tiles; it meets the band iff its smallest offset 256 dt - 255 is <= window"""
    nb = -(-snps // T)
    return sum(nb - dt for dt in range(nb) if T * dt - (T - 1) <= window)


@pytest.mark.parametrize("snps,window", [(s, w) for s in (1, 130, 255, 256, 257, 777, 3000, 5000)
                                         for w in (0, 1, 254, 255, 256, 257, 511, 512, 513, 700, 4999) if w < s])   # window >= snps is an argument error
def test_band_plan_covers_the_band_exactly_once_and_nothing_else(snps, window):
    tiles = ld_band_tiles(snps, window)
    assert len(tiles) == _derived_count(snps, window)
    assert len(set(tiles)) == len(tiles)
    nb = -(-snps // T)
    listed = np.zeros((nb, nb), dtype=np.int64)
    for ti, tj in tiles:
        assert 0 <= ti <= tj < nb
        listed[ti, tj] += 1
    # every element of the band lies in exactly one listed tile
    i = np.arange(snps)[:, None]
    j = i + np.arange(window + 1)[None, :]
    ok = j < snps
    ii, jj = np.broadcast_to(i, j.shape)[ok], j[ok]
    assert np.all(listed[ii // T, jj // T] == 1)
    # no listed tile is wholly outside the band: each holds at least one element of it
    hit = np.zeros((nb, nb), dtype=bool)
    hit[ii // T, jj // T] = True
    assert np.array_equal(hit, listed == 1)


def test_one_more_tile_diagonal_than_window_over_256_unless_the_window_ends_on_a_tile_edge():
    snps = 10 * T
    for window, diagonals in ((0, 1), (1, 2), (255, 2), (256, 2), (257, 3), (511, 3), (512, 3), (513, 4), (1023, 5), (1024, 5)):
        tiles = ld_band_tiles(snps, window)
        assert max(tj - ti for ti, tj in tiles) + 1 == diagonals, window
        assert len(tiles) == sum(10 - dt for dt in range(diagonals)), window


def test_config_2_tile_count():
    """1 000 000 SNPs, window 1023: 3907 tile rows, 5 diagonals"""
    assert len(ld_band_tiles(1_000_000, 1023)) == 5 * 3907 - 10
