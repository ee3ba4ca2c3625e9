"""bench.py --dump-outputs without a GPU: dump_outputs() on a stand-in of the staged workload (host tensors in the layouts stage_headline leaves) writes the
two products as the float64 arrays a caller receives -- whole where they fit the budget, else the same seeded sample of rows every time, with the row numbers
beside it -- from one C_T as from the shards' slices of the in-process form, and stays below 64 MB at the benchmark's default size."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _workload(snps, indiv, n, shards=None):
    g = torch.Generator().manual_seed(7)
    W = types.SimpleNamespace(torch=torch, dist=torch.distributed, rank=0, device=torch.device("cpu"), begin=0, end=snps, inprocess=shards is not None)
    W.C_N = torch.randn((n, indiv), dtype=torch.float64, generator=g).t()          # indiv x n, column-major (stage_headline)
    C_T = torch.randn((n, snps), dtype=torch.float64, generator=g).t()             # snps x n
    if shards:
        W.bounds, W.CT_s = shards, []
        ld = max(e - b for b, e in shards)
        for b, e in shards:                                                         # per shard: ld-padded, column-major, cut to its rows
            buf = torch.zeros((n, ld), dtype=torch.float64)
            buf[:, : e - b] = C_T[b:e].t()
            W.CT_s.append(buf.t()[: e - b])
    else:
        W.C_T = C_T
    return W, C_T.numpy()


def _dump(W, where, snps, indiv, n):
    bench.dump_outputs(W, types.SimpleNamespace(snps=snps, indiv=indiv, ncol=n, dump_outputs=str(where)))
    return {f[:-4]: np.load(where / f) for f in os.listdir(where)}


def test_dump_writes_whole_results_where_they_fit(tmp_path):
    W, C_T = _workload(1003, 501, 4)
    got = _dump(W, tmp_path, 1003, 501, 4)
    assert sorted(got) == ["C_N", "C_T"]
    assert got["C_N"].dtype == got["C_T"].dtype == np.float64 and got["C_N"].shape == (501, 4) and got["C_T"].shape == (1003, 4)
    assert np.array_equal(got["C_N"], W.C_N.numpy()) and np.array_equal(got["C_T"], C_T)


def test_dump_samples_rows_beyond_the_budget_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 40_000)
    snps, indiv, n = 4001, 201, 8                      # 8 n (snps + indiv) = 269 kB > 40 kB; half the budget holds 277 rows + row numbers
    W, C_T = _workload(snps, indiv, n)
    got = _dump(W, tmp_path / "a", snps, indiv, n)
    assert sorted(got) == ["C_N", "C_T", "C_T_rows"]
    rows = got["C_T_rows"]
    assert rows.dtype == np.float64 and len(rows) == 277 and np.all(np.diff(rows) > 0) and rows[-1] < snps and np.array_equal(rows, np.round(rows))
    assert np.array_equal(got["C_T"], C_T[rows.astype(np.int64)]) and np.array_equal(got["C_N"], W.C_N.numpy())
    assert sum(a.nbytes for a in got.values()) <= 40_000
    again = _dump(_workload(snps, indiv, n)[0], tmp_path / "b", snps, indiv, n)
    assert all(np.array_equal(got[k], again[k]) for k in got)
    # the in-process form: the same rows, read from the shard that owns them
    shards = _dump(_workload(snps, indiv, n, shards=[(0, 2000), (2000, 4001)])[0], tmp_path / "c", snps, indiv, n)
    assert all(np.array_equal(got[k], shards[k]) for k in got)


def test_dump_stays_below_64_MB_at_the_default_size():
    snps, indiv, n = 1_000_000, 50_000, 32
    assert bench.dump_rows(indiv, n) is None                      # C_N whole
    rows = bench.dump_rows(snps, n)
    assert rows is not None and len(np.unique(rows)) == len(rows)
    assert 8 * n * indiv + (8 * n + 8) * len(rows) <= bench.DUMP_BYTES <= 64e6
