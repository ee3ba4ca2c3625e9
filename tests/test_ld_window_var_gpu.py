"""Windowed LD by distance: mxa_ld_window_rows / _scores and their pairwise-complete pair, over a window given as data -- SNP j >= i is in the window of i
iff j <= last[i] (mxa_ld_window_bounds makes `last` from base pairs, centimorgans, SNP counts and chromosome ends).

Three window families at the shapes of test_ld_band_gpu.py, both engines, host and device pointers:
  fixed        last[i] = min(i + w, snps - 1): the tile set and the summation order of the fixed entries, so the rows are mxa_ld's R bit for bit, the scores are
               mxa_ld_scores' bits, and the pairwise entries are mxa_ld_band_pairwise's / mxa_ld_scores_pairwise's bits (5 % missing and missing-free data).
  chromosomes  lengths 1, 255, 256, 257, 511, 1, 700 and the rest, positions 1000 k inside a chromosome, max_dist 300 000: windows that stop at chromosome
               ends on, before and behind a tile edge.
  clusters     seeded gaps with ties, many gaps above max_dist and 600 SNPs at one position from index 200 on: reaches from 0 to beyond two tiles, tile rows
               of different lengths.
For the last two: every stored entry is mxa_ld's R(i, i + d) bit for bit (both kinds), nothing is written beyond rowptr[snps], and the scores are compared
with math.fsum of the terms t(r), r from mxa_ld, under the bound test_ld_band_gpu.py derives for ANY summation order of m terms: |err| <= m 2^-53 sum|t|, with
m = last[i] - first[i] + 1 the number of terms of that SNP (first[i] = the smallest k with last[k] >= i).  They are identical from run to run, between the
engines and between host and device pointers.  The pairwise r is mxa_ld_band_pairwise's (window = the largest reach) bit for bit -- the r of a pair does not
depend on the window --, its scores obey the same bound with the terms formed from that r and the pair's N_ij of an exact integer numpy product, and neither
depends on MXA_LD_PAIRWISE_SCRATCH_MB."""
import math

import numpy as np
import pytest

from _ld_ref import first_of as _first, pairs as _pairs          # the stored-pair enumeration and first[], shared with the tests from the definition
from _util import make_problem, pack_plink, synth_genotypes

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SHAPES = [(3000, 400), (777, 515), (130, 1031), (5000, 257)]
SENTINEL = -12345.678
PAD = 67                                   # doubles behind rowptr[snps] that must keep the sentinel
CHROM_LENGTHS = (1, 255, 256, 257, 511, 1, 700)


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


# ------------------------------------------------------------------------------------------------------------------ windows and references
def _fixed_last(snps, w):
    return np.minimum(np.arange(snps) + w, snps - 1).astype(np.int32)


def _windows(snps):
    return sorted({w for w in (0, 1, 255, 256, 257, 700, snps - 1) if w < snps})


def _chromosome_window(mx, snps):
    """the issue's chromosomes (cut where snps ends), positions 1000 k inside each, max_dist 300 000"""
    lengths, left = [], snps
    for ln in CHROM_LENGTHS:
        if left > 0:
            lengths.append(min(ln, left))
            left -= lengths[-1]
    if left > 0:
        lengths.append(left)
    chrom = np.repeat(np.arange(len(lengths)), lengths).astype(np.int32)
    pos = np.concatenate([1000.0 * np.arange(ln) for ln in lengths])
    last, rowptr = mx.crossproduct.ld_window_bounds(pos, chrom, max_dist=300_000.0)
    ends = np.cumsum(lengths) - 1
    assert np.array_equal(last[ends], ends)                                     # no window crosses a chromosome end
    assert np.all(last[:-1][np.diff(chrom) == 0] - np.arange(snps - 1)[np.diff(chrom) == 0] >= 1) or snps < 3
    return last, rowptr


def _cluster_window(mx, snps, seed=17):
    """seeded gaps, 30 % of them 0 (ties) and 15 % above max_dist, and a run of SNPs at one position from index 200 on (600 of them where snps allows)"""
    rng = np.random.default_rng(seed)
    max_dist = 1.0
    gaps = rng.exponential(max_dist / 25.0, size=snps)
    gaps[rng.random(snps) < 0.3] = 0.0
    gaps[rng.random(snps) < 0.15] = max_dist * (1.0 + rng.random())
    run = min(600, snps - 201)
    gaps[201: 200 + run] = 0.0
    gaps[200] = gaps[200 + run] = 2.0 * max_dist                                # the run stands alone
    pos = np.cumsum(gaps)
    last, rowptr = mx.crossproduct.ld_window_bounds(pos, None, max_dist=max_dist)
    reach = last - np.arange(snps)
    tiles = mx.crossproduct.ld_window_tiles(last)
    per_row = np.bincount([t[0] for t in tiles], minlength=(snps + 255) // 256)
    # what makes the case worth having
    assert reach.min() == 0 and reach.max() >= 513 and reach[200] == run - 1
    assert np.any(np.diff(per_row[:-1]) != 0), per_row
    return last, rowptr


def _terms(R, indiv, adjust):
    """t(r) with the kernel's operation order (test_ld_band_gpu.py): r2 = r * r; adjusted: r2 - (1 - r2) * (1 / (indiv - 2))"""
    r2 = R * R
    if not adjust:
        return r2
    return r2 - (1.0 - r2) * (1.0 / (float(indiv) - 2.0))


def _terms_pw(R, N, adjust):
    """the pairwise entries' order (test_ld_pairwise_gpu.py): r2 - ((1 - r2) / (N_ij - 2))"""
    r2 = R * R
    if not adjust:
        return r2
    with np.errstate(divide="ignore", invalid="ignore"):
        return r2 - (1.0 - r2) / (N - 2.0)


def _scores_ref(T, last):
    """per SNP: fsum of its terms T[i, first[i] .. last[i]], sum|t| and the number of terms"""
    n = len(last)
    first = _first(last)
    ref, mag = np.empty(n), np.empty(n)
    for i in range(n):
        row = T[i, first[i]: last[i] + 1]
        ref[i] = math.fsum(row)
        mag[i] = math.fsum(np.abs(row))
    return ref, mag, (last - first + 1).astype(np.float64)


def _assert_scores(got, T, last, what):
    ref, mag, m = _scores_ref(T, last)
    err = np.abs(got - ref)
    bound = m * U * mag
    print(f"scores {what}: worst |err| / bound = {float((err / bound).max()):.3f}, terms per SNP {int(m.min())} .. {int(m.max())}")
    assert np.all(err <= bound), (what, float((err / bound).max()))


_CACHE = {}


def _plain_case(mx, snps, indiv):
    """problem without missing codes and mxa_ld's R of it (computed once per shape, read-only)"""
    key = ("plain", snps, indiv)
    if key not in _CACHE:
        prob = make_problem(snps, indiv, 1, seed=snps + indiv)
        R = mx.crossproduct.ld(prob["plink"], snps, indiv, is_plink_format=True, allele_freq=prob["f"])
        R.setflags(write=False)
        _CACHE[key] = (prob["plink"], prob["f"], R)
    return _CACHE[key]


def _pairwise_case(snps, indiv, missing_frac):
    key = ("pw", snps, indiv, missing_frac)
    if key not in _CACHE:
        Z, miss = synth_genotypes(snps, indiv, seed=snps + indiv, missing_frac=missing_frac)
        _CACHE[key] = np.ascontiguousarray(pack_plink(Z.T.copy(), None if miss is None else miss.T.copy()))
    return _CACHE[key]


def _present_counts(X, indiv):
    """N_ij = individuals genotyped at both SNPs, exact: the fp64 product of 0 / 1 matrices sums integers below 2^53"""
    P = np.ascontiguousarray(X, dtype=np.uint8)
    C = np.stack([(P >> (2 * q)) & 3 for q in range(4)], axis=-1).reshape(P.shape[0], -1)[:, :indiv]
    M = (C != 1).astype(np.float64)
    N = M @ M.T
    k = min(8, len(M))
    assert np.array_equal(N[:k], (M[:k].astype(np.int64) @ M.T.astype(np.int64)).astype(np.float64))
    return N


def _call(mx, entry, X, snps, indiv, last, nout, flag, f=None, device=False):
    """a C entry over `last` with an output of nout + PAD doubles pre-filled with a sentinel; returns (rc, error code, output as numpy)"""
    L = mx.lib.check_library_handle()
    p = mx.lib.ptr
    fn = getattr(L, entry)
    plain = not entry.endswith("_pairwise")
    if device:
        import torch
        dev = torch.device("cuda", 0)
        to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        Xd, ld_, fd = to(X), to(last), to(f)
        out = torch.full((nout + PAD,), SENTINEL, dtype=torch.float64, device=dev)
        rc = fn(p(Xd), snps, indiv, p(ld_), p(out), flag, 1, p(fd)) if plain else fn(p(Xd), snps, indiv, p(ld_), p(out), flag)
        torch.cuda.synchronize()
        return rc, L.mxa_last_error(), out.cpu().numpy()
    out = np.full(nout + PAD, SENTINEL, dtype=np.float64)
    rc = fn(p(X), snps, indiv, p(last), p(out), flag, 1, p(f)) if plain else fn(p(X), snps, indiv, p(last), p(out), flag)
    return rc, L.mxa_last_error(), out


def _good(mx, entry, X, snps, indiv, last, nout, flag, f=None, device=False):
    rc, err, out = _call(mx, entry, X, snps, indiv, last, nout, flag, f, device)
    assert (rc, err) == (0, 0), (entry, mx.lib.last_error())
    assert np.all(out[nout:] == SENTINEL), entry                                 # nothing beyond the result
    return out[:nout]


# ------------------------------------------------------------------------------------------------------------------------ 1. fixed windows
@pytest.mark.parametrize("snps,indiv", SHAPES)
@pytest.mark.parametrize("engine", ["f4", "i8"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_fixed_window_gives_the_bits_of_mxa_ld_and_mxa_ld_scores(mx, monkeypatch, snps, indiv, engine, device):
    X, f, R = _plain_case(mx, snps, indiv)
    assert np.isfinite(R).all()
    monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
    for w in _windows(snps):
        last = _fixed_last(snps, w)
        ii, jj = _pairs(last)
        want = R[ii, jj]
        for kind in (0, 1):
            got = _good(mx, "mxa_ld_window_rows", X, snps, indiv, last, len(ii), kind, f, device)
            assert np.array_equal(got, want * want if kind else want), (w, kind)
        for adjust in (0, 1):
            got = _good(mx, "mxa_ld_window_scores", X, snps, indiv, last, snps, adjust, f, device)
            fixed = mx.crossproduct.ld_scores(X, snps, indiv, w, adjust=bool(adjust), is_plink_format=True, allele_freq=f)
            assert np.array_equal(got, fixed), (w, adjust)


@pytest.mark.parametrize("snps,indiv", SHAPES)
@pytest.mark.parametrize("engine", ["f4", "i8"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("missing_frac", [0.05, 0.0], ids=["missing", "missing-free"])
def test_fixed_window_gives_the_bits_of_the_pairwise_entries(mx, monkeypatch, snps, indiv, engine, device, missing_frac):
    X = _pairwise_case(snps, indiv, missing_frac)
    monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
    cp = mx.crossproduct
    for w in _windows(snps):
        last = _fixed_last(snps, w)
        ii, jj = _pairs(last)
        B = cp.ld_band_pairwise(X, snps, indiv, w)
        want = B[ii, jj - ii]
        assert np.isfinite(want).all()
        for kind in (0, 1):
            got = _good(mx, "mxa_ld_window_rows_pairwise", X, snps, indiv, last, len(ii), kind, None, device)
            assert np.array_equal(got, want * want if kind else want), (w, kind)
        for adjust in (0, 1):
            got = _good(mx, "mxa_ld_window_scores_pairwise", X, snps, indiv, last, snps, adjust, None, device)
            assert np.array_equal(got, cp.ld_scores_pairwise(X, snps, indiv, w, adjust=bool(adjust))), (w, adjust)


# -------------------------------------------------------------------------------------------------------- 2. chromosomes and clusters
def _family(mx, family, snps):
    return _chromosome_window(mx, snps) if family == "chromosomes" else _cluster_window(mx, snps)


FAMILY_CASES = [("chromosomes", s, n) for s, n in SHAPES] + [("clusters", s, n) for s, n in SHAPES if s >= 777]   # a reach of 513 needs more than 130 SNPs


def test_the_chromosome_family_at_3000_snps_is_the_one_described():
    import miraculix_amd as m
    last, rowptr = _chromosome_window(m, 3000)
    chrom_end = np.cumsum(CHROM_LENGTHS + (3000 - sum(CHROM_LENGTHS),)) - 1
    assert chrom_end.tolist() == [0, 255, 511, 768, 1279, 1280, 1980, 2999]
    reach = last - np.arange(3000)
    assert reach.max() == 300 and reach.min() == 0 and rowptr[-1] == int((reach + 1).sum())


@pytest.mark.parametrize("family,snps,indiv", FAMILY_CASES)
def test_rows_equal_mxa_ld_bit_for_bit_and_nothing_is_written_beyond_them(mx, monkeypatch, family, snps, indiv):
    X, f, R = _plain_case(mx, snps, indiv)
    assert np.isfinite(R).all()
    last, rowptr = _family(mx, family, snps)
    ii, jj = _pairs(last)
    assert len(ii) == rowptr[-1] and np.array_equal(rowptr[ii] + (jj - ii), np.arange(len(ii)))     # rows[rowptr[i] + d] = R(i, i + d)
    want = R[ii, jj]
    for engine in ("f4", "i8"):
        monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
        for device in (False, True):
            for kind in (0, 1):
                got = _good(mx, "mxa_ld_window_rows", X, snps, indiv, last, len(ii), kind, f, device)
                assert np.array_equal(got, want * want if kind else want), (engine, device, kind)
    # the Python binding: numpy in -> numpy out, device tensor in -> device tensor out
    import torch
    dev = torch.device("cuda", 0)
    Bn = mx.crossproduct.ld_window_rows(X, snps, indiv, last, kind="r2", is_plink_format=True, allele_freq=f)
    Bd = mx.crossproduct.ld_window_rows(torch.from_numpy(X).to(dev), snps, indiv, torch.from_numpy(last).to(dev), kind="r2", is_plink_format=True,
                                        allele_freq=torch.from_numpy(f).to(dev))
    assert isinstance(Bn, np.ndarray) and Bn.shape == (rowptr[-1],) and Bd.is_cuda and np.array_equal(Bn, want * want) and np.array_equal(Bd.cpu().numpy(), Bn)


@pytest.mark.parametrize("family,snps,indiv", FAMILY_CASES)
def test_scores_within_the_summation_bound_and_reproducible(mx, monkeypatch, family, snps, indiv):
    X, f, R = _plain_case(mx, snps, indiv)
    assert np.isfinite(R).all()
    last, _ = _family(mx, family, snps)
    import torch
    dev = torch.device("cuda", 0)
    Xd, fd, lastd = torch.from_numpy(X).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(last).to(dev)
    cp = mx.crossproduct
    for adjust in (False, True):
        got = {}
        for engine in ("f4", "i8"):
            monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
            a = _good(mx, "mxa_ld_window_scores", X, snps, indiv, last, snps, int(adjust), f, False)
            b = cp.ld_window_scores(X, snps, indiv, last, adjust=adjust, is_plink_format=True, allele_freq=f)
            assert isinstance(b, np.ndarray) and b.shape == (snps,)
            assert np.array_equal(a, b), (engine, adjust)                                   # run to run
            d = cp.ld_window_scores(Xd, snps, indiv, lastd, adjust=adjust, is_plink_format=True, allele_freq=fd)
            assert d.is_cuda and np.array_equal(d.cpu().numpy(), a), (engine, adjust)       # device pointers
            got[engine] = a
        assert np.array_equal(got["f4"], got["i8"]), adjust                                 # engine to engine
        _assert_scores(got["f4"], _terms(R, indiv, adjust), last, f"{family} {snps}x{indiv} adjust={adjust}")


@pytest.mark.parametrize("family,snps,indiv", FAMILY_CASES)
def test_pairwise_rows_and_scores_against_the_fixed_band_and_the_summation_bound(mx, monkeypatch, family, snps, indiv):
    X = _pairwise_case(snps, indiv, 0.05)
    last, rowptr = _family(mx, family, snps)
    ii, jj = _pairs(last)
    reach = int((last - np.arange(snps)).max())
    cp = mx.crossproduct
    monkeypatch.setenv("MXA_XPROD_ENGINE", "f4")
    monkeypatch.delenv("MXA_LD_PAIRWISE_SCRATCH_MB", raising=False)
    want = cp.ld_band_pairwise(X, snps, indiv, reach)[ii, jj - ii]                  # the r of a pair does not depend on the window
    assert np.isfinite(want).all()
    rows, scores = {}, {}
    for engine in ("f4", "i8"):
        monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
        for cap in (None, "1"):                                                     # one group / one tile row per group
            if cap is None:
                monkeypatch.delenv("MXA_LD_PAIRWISE_SCRATCH_MB", raising=False)
            else:
                monkeypatch.setenv("MXA_LD_PAIRWISE_SCRATCH_MB", cap)
            for device in (False, True):
                for kind in (0, 1):
                    got = _good(mx, "mxa_ld_window_rows_pairwise", X, snps, indiv, last, len(ii), kind, None, device)
                    assert np.array_equal(got, want * want if kind else want), (engine, cap, device, kind)
                for adjust in (0, 1):
                    s = _good(mx, "mxa_ld_window_scores_pairwise", X, snps, indiv, last, snps, adjust, None, device)
                    assert np.array_equal(s, scores.setdefault(adjust, s)), (engine, cap, device, adjust)
    monkeypatch.delenv("MXA_LD_PAIRWISE_SCRATCH_MB", raising=False)
    # the bound: the terms from the stored r itself and the exact N_ij
    N = _present_counts(X, indiv)
    Rfull = np.full((snps, snps), np.nan)
    Rfull[ii, jj] = want
    Rfull[jj, ii] = want
    for adjust in (0, 1):
        _assert_scores(scores[adjust], _terms_pw(Rfull, N, bool(adjust)), last, f"pairwise {family} {snps}x{indiv} adjust={adjust}")
    import torch
    dev = torch.device("cuda", 0)
    Sd = cp.ld_window_scores_pairwise(torch.from_numpy(X).to(dev), snps, indiv, torch.from_numpy(last).to(dev), adjust=True)
    Bn = cp.ld_window_rows_pairwise(X, snps, indiv, last)
    assert Sd.is_cuda and np.array_equal(Sd.cpu().numpy(), scores[1]) and isinstance(Bn, np.ndarray) and np.array_equal(Bn, want)


def test_missing_free_pairwise_input_takes_the_fast_path_with_the_same_bits(mx, monkeypatch):
    snps, indiv = 3000, 400
    X = _pairwise_case(snps, indiv, 0.0)
    last, _ = _cluster_window(mx, snps)
    ii, _ = _pairs(last)
    for engine in ("f4", "i8"):
        monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
        monkeypatch.delenv("MXA_LD_PAIRWISE_DENSE", raising=False)
        fast = [_good(mx, "mxa_ld_window_rows_pairwise", X, snps, indiv, last, len(ii), 0)] + \
               [_good(mx, "mxa_ld_window_scores_pairwise", X, snps, indiv, last, snps, a) for a in (0, 1)]
        monkeypatch.setenv("MXA_LD_PAIRWISE_DENSE", "1")
        six = [_good(mx, "mxa_ld_window_rows_pairwise", X, snps, indiv, last, len(ii), 0)] + \
              [_good(mx, "mxa_ld_window_scores_pairwise", X, snps, indiv, last, snps, a) for a in (0, 1)]
        for a, b in zip(fast, six):
            assert np.isfinite(a).all() and np.array_equal(a, b), engine


def test_a_monomorphic_snp_gives_the_non_finite_entries_of_mxa_ld(mx):
    snps, indiv = 777, 515
    prob = make_problem(snps, indiv, 1, seed=6)
    Z = prob["Z"].copy()
    mono = 256                                         # first SNP of the second tile
    Z[:, mono] = 0
    X = pack_plink(np.ascontiguousarray(Z.T))
    f = Z.astype(np.float64).mean(axis=0) / 2.0
    R = mx.crossproduct.ld(X, snps, indiv, is_plink_format=True, allele_freq=f)
    assert not np.isfinite(R[mono]).any() and np.isfinite(np.delete(np.delete(R, mono, 0), mono, 1)).all()
    last, _ = _chromosome_window(mx, snps)
    ii, jj = _pairs(last)
    got = _good(mx, "mxa_ld_window_rows", X, snps, indiv, last, len(ii), 0, f)
    assert np.array_equal(got, R[ii, jj], equal_nan=True) and not np.isfinite(got[(ii == mono) | (jj == mono)]).any()
    S = mx.crossproduct.ld_window_scores(X, snps, indiv, last, is_plink_format=True, allele_freq=f)
    first = _first(last)
    near = (first <= mono) & (mono <= last)
    assert near.sum() > 1 and not np.isfinite(S[near]).any() and np.isfinite(S[~near]).all()


# ---------------------------------------------------------------------------------------------------------------------------- 3. arguments
def test_bad_arguments_return_one_and_leave_the_output_untouched(mx):
    snps, indiv = 300, 40
    prob = make_problem(snps, indiv, 1, seed=9)
    X, f = prob["plink"], prob["f"]
    good = _fixed_last(snps, 10)
    L = mx.lib.check_library_handle()
    p = mx.lib.ptr
    bad = (1, 1, True)

    def run(entry, Xs=X, nind=indiv, last=good, flag=0, freq=f, with_out=True, n=snps):
        out = np.full(4000, SENTINEL)
        fn = getattr(L, entry)
        o = p(out) if with_out else None
        rc = fn(p(Xs), n, nind, p(last), o, flag) if entry.endswith("_pairwise") else fn(p(Xs), n, nind, p(last), o, flag, 1, p(freq))
        return rc, L.mxa_last_error(), bool(np.all(out == SENTINEL))

    def changed(i, v):
        a = good.copy()
        a[i] = v
        return a

    X2 = np.ascontiguousarray(X[:, :1])                # 2 individuals: one byte per SNP
    for entry in ("mxa_ld_window_rows", "mxa_ld_window_scores", "mxa_ld_window_rows_pairwise", "mxa_ld_window_scores_pairwise"):
        assert run(entry, Xs=None) == bad and run(entry, last=None) == bad and run(entry, with_out=False) == bad, entry
        assert run(entry, n=0) == bad and run(entry, nind=0) == bad, entry
        assert run(entry, last=changed(5, 4)) == bad, entry                       # last[i] < i
        assert run(entry, last=changed(snps - 1, snps)) == bad, entry             # last[i] >= snps
        assert run(entry, last=changed(0, -1)) == bad, entry
        assert run(entry, last=changed(7, 30)) == bad, entry                      # decreasing behind it
        assert run(entry, flag=2) == bad and run(entry, flag=-1) == bad, entry    # kind / adjust
        if "scores" in entry:
            assert run(entry, Xs=X2, nind=2, flag=1) == bad, entry                # the adjusted estimator needs indiv >= 3
            assert run(entry, Xs=X2, nind=2, flag=0)[:2] == (0, 0), entry
        if entry.endswith("_pairwise"):
            assert run(entry, nind=47_453_133) == bad, entry                      # 4 indiv^2 >= 2^53
        else:
            assert run(entry, freq=None) == bad, entry
        assert run(entry) == (0, 0, False), entry                                 # the process is alive and the next good call succeeds
    # the same through a device `last`
    import torch
    out = np.full(4000, SENTINEL)
    rc = L.mxa_ld_window_rows(p(X), snps, indiv, p(torch.from_numpy(changed(7, 30)).to("cuda:0")), p(out), 0, 1, p(f))
    assert (rc, L.mxa_last_error(), bool(np.all(out == SENTINEL))) == bad
    with pytest.raises(ValueError):
        mx.crossproduct.ld_window_rows(X, snps, indiv, changed(7, 30), is_plink_format=True, allele_freq=f)
    with pytest.raises(ValueError):
        mx.crossproduct.ld_window_rows(X, snps, indiv, good, kind="r3", is_plink_format=True, allele_freq=f)
    with pytest.raises(ValueError):
        mx.crossproduct.ld_window_scores(X, snps, indiv, good, is_plink_format=True, allele_freq=None)
    with pytest.raises(ValueError):
        mx.crossproduct.ld_window_scores_pairwise(X2, snps, 2, good, adjust=True)


# ------------------------------------------------------------------------------------------------------ the gang form of the kernels
def test_rows_and_scores_do_not_depend_on_the_kernel_form():
    """As test_ld_band_gpu.py does for the fixed entries: MXA_XPROD_GANG=2 forces the gang-synchronised persistent kernel wherever the tile list is long enough
    for the per-XCD lists (30 000 SNPs under a clustered window of at least 512 tiles, asserted), also with the XCD id masked so that lists are stolen.  In
    every form the rows equal mxa_ld's R bit for bit, and rows and scores -- the pairwise ones too -- are the same bits in all three forms and on both
    engines.  The knobs are read once per process: a child process per setting."""
    import os
    import subprocess
    import sys
    code = """
import sys, os, hashlib, numpy as np, torch
sys.path.insert(0, %r)
import miraculix_amd as mx
mx.load_shared_library()
dev = torch.device("cuda", 0)
snps, indiv = 30000, 300
rng = np.random.default_rng(4)
p = rng.uniform(0.1, 0.6, size=snps)
Z = rng.binomial(2, p[:, None], size=(snps, indiv)).astype(np.uint8)
code = np.where(Z == 0, 0, Z + 1).astype(np.uint8)
def pack(c):
    c = c.reshape(snps, -1, 4)
    return torch.from_numpy(np.ascontiguousarray(c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6))).to(dev)
X = pack(code)
miss = code.copy()
miss[rng.random((snps, indiv)) < 0.05] = 1
Xm = pack(miss)
f = torch.from_numpy(Z.astype(np.float64).mean(axis=1) / 2.0).to(dev)
# a clustered window: regions of 3000 SNPs whose density alternates 1 : 3, ties, gaps above max_dist, 600 SNPs at one position from index 200 on
gaps = rng.exponential(1.0, size=snps) * np.where((np.arange(snps) // 3000) %% 2 == 0, 1.0, 3.0)
gaps[rng.random(snps) < 0.2] = 0.0
gaps[rng.random(snps) < 0.0003] = 3000.0
gaps[201:800] = 0.0
cp = mx.crossproduct
last, rowptr = cp.ld_window_bounds(np.cumsum(gaps), None, max_dist=1500.0)
reach = last - np.arange(snps)
ntiles = len(cp.ld_window_tiles(last))
assert ntiles >= 512 and reach.min() == 0 and reach.max() >= 513, (ntiles, reach.min(), reach.max())
lastd = torch.from_numpy(last).to(dev)
cnt = torch.from_numpy(reach.astype(np.int64) + 1).to(dev)
ii = torch.repeat_interleave(torch.arange(snps, device=dev), cnt)
jj = ii + (torch.arange(ii.numel(), device=dev) - torch.repeat_interleave(torch.from_numpy(rowptr[:-1]).to(dev), cnt))
R = cp.ld(X, snps, indiv, is_plink_format=True, allele_freq=f)
want = R[ii, jj]
del R
h = []
for eng in ("f4", "i8"):
    os.environ["MXA_XPROD_ENGINE"] = eng
    B = cp.ld_window_rows(X, snps, indiv, lastd, is_plink_format=True, allele_freq=f)
    assert torch.equal(B, want), eng
    he = []
    for adjust in (False, True):
        S = cp.ld_window_scores(X, snps, indiv, lastd, adjust=adjust, is_plink_format=True, allele_freq=f)
        assert bool(torch.isfinite(S).all())
        he.append(hashlib.sha256(S.cpu().numpy().tobytes()).hexdigest())
    Bp = cp.ld_window_rows_pairwise(Xm, snps, indiv, lastd)
    assert bool(torch.isfinite(Bp).all())
    he.append(hashlib.sha256(Bp.cpu().numpy().tobytes()).hexdigest())
    for adjust in (False, True):
        he.append(hashlib.sha256(cp.ld_window_scores_pairwise(Xm, snps, indiv, lastd, adjust=adjust).cpu().numpy().tobytes()).hexdigest())
    h.append(he)
assert h[0] == h[1], "FP4 and int8 differ"
print("hashes", ntiles, *h[0])
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),)
    seen = set()
    for env in ({"MXA_XPROD_GANG": "0"}, {"MXA_XPROD_GANG": "2"}, {"MXA_XPROD_GANG": "2", "MXA_XPROD_GANG_XCC_MASK": "1"}):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("hashes ")]
        assert r.returncode == 0 and len(lines) == 1, (env, r.stdout + r.stderr)
        seen.add(lines[0])
    assert len(seen) == 1, seen
