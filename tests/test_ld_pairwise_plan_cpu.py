"""The tile plan of the pairwise-complete windowed LD entries (mxa_ld_band_pairwise, mxa_ld_scores_pairwise), restated in
miraculix_amd.crossproduct.ld_pairwise_tiles: the band tiles of ld_band_tiles in groups of tile rows; per band tile (I, J) the six products
(M, M), (Z, Z), (Z, M), (M, Z), (A, M), (M, A) over the stacked operand of 3 nb row blocks (x = plane_a nb + I, y = plane_b nb + J), each with a scratch
slot of its own within the group.  Checked here: every band tile gets the six pairs exactly once (the library keeps all six on diagonal tiles too), no entry
lies outside the band, the stacked indices stay below 3 nb, slots are dense and distinct within a group, and groups chosen by ld_pairwise_group_rows respect
the scratch cap (one tile row at least).  The library's planner is the same loops in C++; the GPU tests check its results element by element."""
import pytest

from miraculix_amd.crossproduct import (PAIRWISE_PAIRS, PAIRWISE_PLANES, PAIRWISE_SLOT_BYTES, ld_band_tiles, ld_pairwise_group_rows, ld_pairwise_tiles)

T = 256
CASES = [(s, w) for s in (1, 130, 255, 256, 257, 777, 3000, 5000) for w in (0, 1, 255, 256, 257, 700, 4999) if w < s]


def test_the_six_pairs_are_the_sums_of_the_formula():
    """slot order N, Sxy, Sx, Sy, sum a_i m_j, sum m_i a_j: the I rows give the first factor, the J rows the second"""
    assert PAIRWISE_PAIRS == (("M", "M"), ("Z", "Z"), ("Z", "M"), ("M", "Z"), ("A", "M"), ("M", "A"))
    assert sorted(PAIRWISE_PLANES.values()) == [0, 1, 2]
    assert PAIRWISE_SLOT_BYTES == T * T * 4


@pytest.mark.parametrize("snps,window", CASES)
@pytest.mark.parametrize("group", [1, 2, 3, 1000])
def test_every_band_tile_gets_the_six_pairs_once_and_nothing_lies_outside_the_band(snps, window, group):
    nb = -(-snps // T)
    band = ld_band_tiles(snps, window)
    groups = ld_pairwise_tiles(snps, window, group)
    assert len(groups) == -(-nb // group)
    want_pairs = sorted((PAIRWISE_PLANES[a], PAIRWISE_PLANES[b]) for a, b in PAIRWISE_PAIRS)
    seen = {}
    for gi, entries in enumerate(groups):
        slots = sorted(slot for _, _, slot in entries)
        assert slots == list(range(len(entries))) and len(entries) % 6 == 0          # dense and distinct within the group
        for x, y, slot in entries:
            assert 0 <= x < 3 * nb and 0 <= y < 3 * nb
            pa, i, pb, j = x // nb, x % nb, y // nb, y % nb
            assert gi * group <= i < (gi + 1) * group                                # a group is a range of tile rows
            seen.setdefault((i, j), []).append((pa, pb, slot))
    assert sorted(seen) == sorted(band)                                              # the band's tiles, no other
    for (i, j), lst in seen.items():
        assert sorted((pa, pb) for pa, pb, _ in lst) == want_pairs, (i, j)
        base = min(slot for _, _, slot in lst)
        assert base % 6 == 0 and [(PAIRWISE_PLANES[a], PAIRWISE_PLANES[b], base + k) for k, (a, b) in enumerate(PAIRWISE_PAIRS)] == lst   # slot order = pair order


@pytest.mark.parametrize("snps,window", CASES + [(1_000_000, 1023)])
@pytest.mark.parametrize("scratch_mb", [1, 2, 12, 40, 2048])
def test_groups_respect_the_scratch_cap(snps, window, scratch_mb):
    nb = -(-snps // T)
    rows = ld_pairwise_group_rows(snps, window, scratch_mb)
    assert 1 <= rows <= nb
    row_tiles = min(nb, -(-window // T) + 1)
    one_row = row_tiles * 6 * PAIRWISE_SLOT_BYTES
    if snps <= 5000:
        worst = max(len(g) for g in ld_pairwise_tiles(snps, window, rows)) * PAIRWISE_SLOT_BYTES
        assert worst <= max(scratch_mb << 20, one_row)
    else:
        assert rows * one_row <= max(scratch_mb << 20, one_row)
    if rows < nb:                                                                    # and one more tile row would not have fitted
        assert (rows + 1) * one_row > scratch_mb << 20


def test_config_2_plan():
    """1 000 000 SNPs, window 1023: 5 tiles per tile row, 7.5 MiB of counts each: 273 tile rows per group under the 2 GiB default, 15 groups; the fast path
    (one product per band tile) fits 1638 tile rows"""
    assert ld_pairwise_group_rows(1_000_000, 1023) == 273
    assert -(-3907 // 273) == 15
    assert ld_pairwise_group_rows(1_000_000, 1023, pairs=1) == 1638
