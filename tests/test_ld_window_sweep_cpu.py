"""The seeded window geometries of tests/test_ld_window_edges_gpu.py (snps = 700, 32 seeds) hold every event they are there for -- no GPU needed: the
generator and the events are plain numpy (tests/_ld_ref.py)."""
from collections import Counter

import numpy as np

from _ld_ref import SWEEP_EVENTS, first_of, pairs, rowptr_of, sweep_events, sweep_window

SNPS, SEEDS = 700, 32


def test_every_window_event_occurs_over_the_seeds():
    seen = Counter()
    for seed in range(SEEDS):
        last = sweep_window(SNPS, seed)
        assert last.dtype == np.int32 and np.array_equal(last, sweep_window(SNPS, seed))       # seeded: the same window every time
        seen.update(sweep_events(last))
    print({e: seen[e] for e in SWEEP_EVENTS})
    assert set(seen) <= set(SWEEP_EVENTS)
    for e in SWEEP_EVENTS:
        assert seen[e] >= 1, e


def test_the_pair_enumeration_agrees_with_rowptr_and_first():
    last = sweep_window(SNPS, 5)
    ii, jj = pairs(last)
    rowptr = rowptr_of(last)
    assert len(ii) == rowptr[-1] and np.array_equal(rowptr[ii] + (jj - ii), np.arange(len(ii)))
    first = first_of(last)
    for i in (0, 1, 255, 256, 699):
        assert first[i] == min(k for k in range(SNPS) if last[k] >= i)
