"""Pairwise-complete windowed LD on data with missing genotypes: mxa_ld_band_pairwise / mxa_ld_scores_pairwise.

The reference for every value is the numpy restatement of tests/_ld_ref.py (pairwise_restate), from the unpacked PLINK codes: m = present, z = allele count with missing as 0,
a = code 11; N = M M^T, Sxy = Z Z^T, Sx = Z M^T, Sy = Sx^T, Sxx = Sx + 2 A M^T, Syy = Sxx^T as int64 matrices; num = N Sxy - Sx Sy, dx = N Sxx - Sx^2,
dy = dx^T in int64; r_ref = num / sqrt(dx dy) in np.longdouble.  (The matrix products run through the fp64 BLAS and are converted to int64: every partial
sum is an integer below 4 * 1031 < 2^53, so they are the int64 products; a block of rows is recomputed with numpy's own int64 product and must be equal.)
Neither mxa_ld nor the code under test enters the reference.

Band tolerance: |r - r_ref| <= 8 * 2^-53 * |r_ref|.  The integers are exact, and any sensible order of the remaining operations (dx dy, square root, quotient,
or reciprocals instead) has at most six roundings of 2^-53 each; the library's order num / sqrt(dx dy) has three, the square root's halved.  No entry of the
restatement is non-finite at the four shapes (asserted), so every in-band entry is compared.  kind 1 is r * r with one rounding: compared bit for bit with
the square of the kind-0 band.  Engines, pointer kinds, scratch caps and the missing-free fast path must all give the same bits.
Scores: math.fsum of the terms formed from the band entry's own r (and the restatement's exact N_ij for adjust), under the any-order bound of
test_ld_band_gpu.py: |err| <= m 2^-53 sum|t|, m = 2 window + 1."""
import math

import numpy as np
import pytest

from _ld_ref import PAIRWISE_UNITS, codes, pairwise_restate
from _util import pack_plink, synth_genotypes

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SHAPES = [(3000, 400), (777, 515), (130, 1031), (5000, 257)]
SENTINEL = -12345.678
LD = np.longdouble


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


def _windows(snps):
    return sorted({w for w in (0, 1, 255, 256, 257, 700, snps - 1) if w < snps})


def _problem(snps, indiv, missing_frac):
    Z, miss = synth_genotypes(snps, indiv, seed=snps + indiv, missing_frac=missing_frac)
    return np.ascontiguousarray(pack_plink(Z.T.copy(), None if miss is None else miss.T.copy()))


def _codes(plink, indiv):
    return codes(plink, indiv)


def _restate(plink, indiv):
    """dict(N, Sxy: int64 snps x snps; r: longdouble, NaN where dx dy = 0) -- the formulas of the issue on the unpacked codes (tests/_ld_ref.py)"""
    return pairwise_restate(plink, indiv)


def _band_of(R, window, fill=0.0):
    """the band storage of a full matrix: out[i, d] = R[i, i + d], `fill` where i + d >= snps"""
    n = R.shape[0]
    idx = np.arange(n)[:, None] + np.arange(window + 1)[None, :]
    return np.where(idx < n, R[np.arange(n)[:, None], np.minimum(idx, n - 1)], fill)


def _call_band(mx, X, snps, indiv, window, ldb, kind, device):
    """the C entry with a band of leading dimension ldb pre-filled with a sentinel; returns (rc, band as a numpy (snps, ldb) array)"""
    L = mx.lib.check_library_handle()
    if device:
        import torch
        dev = torch.device("cuda", 0)
        Xd = torch.from_numpy(X).to(dev)
        B = torch.full((snps, ldb), SENTINEL, dtype=torch.float64, device=dev)
        rc = L.mxa_ld_band_pairwise(mx.lib.ptr(Xd), snps, indiv, window, mx.lib.ptr(B), ldb, kind)
        torch.cuda.synchronize()
        return rc, B.cpu().numpy()
    B = np.full((snps, ldb), SENTINEL, dtype=np.float64)
    rc = L.mxa_ld_band_pairwise(mx.lib.ptr(X), snps, indiv, window, mx.lib.ptr(B), ldb, kind)
    return rc, B


def _assert_band(B, ref_r, window, what):
    """every in-band entry within 8 units of 2^-53 of the restatement, NaN exactly where it is NaN; +0.0 in the tail; the sentinel beyond the window"""
    snps = ref_r.shape[0]
    got = B[:, : window + 1]
    inband = (np.arange(snps)[:, None] + np.arange(window + 1)[None, :]) < snps
    want = _band_of(ref_r, window, fill=LD(0))
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    ok = inband & ~nan
    err = np.abs(got.astype(LD) - want)[ok]
    unit = (U * np.abs(want))[ok]
    worst = float((err / np.where(unit > 0, unit, 1)).max()) if err.size else 0.0
    print(f"band {what}: worst |r - r_ref| = {worst:.2f} units of 2^-53 |r_ref| over {int(ok.sum())} entries")
    assert np.all(err <= PAIRWISE_UNITS * unit), (what, worst)
    assert np.all(got[~inband] == 0.0) and not np.signbit(got[~inband]).any(), what
    assert np.all(B[:, window + 1:] == SENTINEL), what


# ------------------------------------------------------------------------------------------------------- 1. the band against the restatement
@pytest.mark.parametrize("snps,indiv", SHAPES)
@pytest.mark.parametrize("missing_frac", [0.05, 0.3])
def test_band_against_the_numpy_restatement(mx, monkeypatch, snps, indiv, missing_frac):
    X = _problem(snps, indiv, missing_frac)
    assert (_codes(X, indiv) == 1).any()
    ref = _restate(X, indiv)
    assert np.isfinite(ref["r"]).all() and ref["N"].min() >= 84          # nothing is left out below
    for window in _windows(snps):
        ldb = window + 4
        first = {}
        for engine in ("f4", "i8"):
            monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
            for device in (False, True):
                for kind in (0, 1):
                    rc, B = _call_band(mx, X, snps, indiv, window, ldb, kind, device)
                    assert rc == 0, (window, kind, engine, device, mx.lib.last_error())
                    what = f"{snps}x{indiv} miss={missing_frac} window={window} kind={kind} {engine} {'device' if device else 'host'}"
                    if kind not in first:
                        first[kind] = B
                        if kind == 0:
                            _assert_band(B, ref["r"], window, what)
                        else:                                                     # r * r, one rounding, of the kind-0 entry
                            assert np.array_equal(B[:, : window + 1], first[0][:, : window + 1] * first[0][:, : window + 1]), what
                            assert np.all(B[:, window + 1:] == SENTINEL), what
                    else:                                                         # the other engine / pointer kind: the same bits
                        assert np.array_equal(B, first[kind]), what
    # the Python binding: shape (snps, window + 1), numpy in -> numpy out, device tensor in -> device tensor out
    import torch
    w = min(257, snps - 1)
    Bn = mx.crossproduct.ld_band_pairwise(X, snps, indiv, w, kind="r2")
    Bd = mx.crossproduct.ld_band_pairwise(torch.from_numpy(X).to("cuda:0"), snps, indiv, w, kind="r2")
    assert isinstance(Bn, np.ndarray) and Bn.shape == (snps, w + 1) and Bd.is_cuda and np.array_equal(Bd.cpu().numpy(), Bn)
    r = _band_of(ref["r"], w, fill=LD(0)).astype(np.float64)
    assert np.allclose(Bn, r * r, rtol=1e-14, atol=0)


# ---------------------------------------------------------------------------------------------------------------------- 2. degenerate pairs
def _degenerate_codes():
    """40 SNPs x 37 individuals (37 % 4 = 1) of PLINK codes: SNP 0 missing everywhere; SNPs 1 and 2 without a shared individual; SNP 3 constant (code 10) on
    the individuals it shares with SNP 4 but not elsewhere; SNP 5 monomorphic; the rest random with 20 % missing"""
    snps, indiv = 40, 37
    rng = np.random.default_rng(11)
    C = rng.choice(np.array([0, 2, 3], dtype=np.uint8), size=(snps, indiv))
    C[rng.random((snps, indiv)) < 0.2] = 1
    C[0] = 1
    C[1, 18:] = 1
    C[1, :18] = rng.choice(np.array([0, 2, 3], dtype=np.uint8), size=18)
    C[2, :18] = 1
    C[2, 18:] = rng.choice(np.array([0, 2, 3], dtype=np.uint8), size=19)
    C[4, :20] = 1
    C[4, 20:] = rng.choice(np.array([0, 2, 3], dtype=np.uint8), size=17)
    C[3, 20:] = 2
    C[3, :20] = rng.choice(np.array([0, 2, 3], dtype=np.uint8), size=20)
    C[5] = 3
    return C


def _pack_codes(C, pad_code=0):
    rows, cols = C.shape
    pad = (-cols) % 4
    Cp = np.concatenate([C, np.full((rows, pad), pad_code, np.uint8)], axis=1).reshape(rows, -1, 4)
    return np.ascontiguousarray((Cp[:, :, 0] | (Cp[:, :, 1] << 2) | (Cp[:, :, 2] << 4) | (Cp[:, :, 3] << 6)).astype(np.uint8))


@pytest.mark.parametrize("engine", ["f4", "i8"])
def test_degenerate_pairs_are_nan_exactly_where_the_restatement_is(mx, monkeypatch, engine):
    monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
    C = _degenerate_codes()
    snps, indiv = C.shape
    X = _pack_codes(C)
    ref = _restate(X, indiv)
    nan = np.isnan(ref["r"])
    assert nan[0].all() and nan[1, 2] and nan[3, 4] and nan[5].all() and not nan[1, 1] and not nan[3, 3] and not nan[6:, 6:].all()
    assert ref["N"][1, 2] == 0 and ref["N"][3, 4] == 17
    window = snps - 1
    for device in (False, True):
        rc, B = _call_band(mx, X, snps, indiv, window, window + 4, 0, device)
        assert rc == 0
        _assert_band(B, ref["r"], window, f"degenerate {engine} device={device}")
    # the padding bits of a row's last byte are not individuals, whatever they hold: the same bits with 01 / 11 there
    for pad_code in (1, 3):
        rc, B2 = _call_band(mx, _pack_codes(C, pad_code), snps, indiv, window, window + 4, 0, False)
        assert rc == 0 and np.array_equal(B2, B, equal_nan=True), pad_code
    # scores: non-finite exactly where the window holds a NaN pair
    S = mx.crossproduct.ld_scores_pairwise(X, snps, indiv, 3)
    hit = np.array([nan[i, max(0, i - 3): i + 4].any() for i in range(snps)])
    assert np.array_equal(~np.isfinite(S), hit)


# ------------------------------------------------------------------------------------------------------------------------------- 3. scores
def _terms(r, N, adjust):
    """t(r) with the library's operation order, every operation rounded on its own: r2 = r * r; adjusted: r2 - ((1 - r2) / (N - 2))"""
    r2 = r * r
    if not adjust:
        return r2
    return r2 - (1.0 - r2) / (N.astype(np.float64) - 2.0)


def _scores_ref(B, Nband, window, adjust):
    """per SNP: fsum of the terms within the window (from the band entries' own r), and sum|t|"""
    n = B.shape[0]
    T = _terms(B, Nband, adjust)                                # T[i, d] = t(r(i, i + d)); entries with i + d >= n are not read below
    ref, mag = np.empty(n), np.empty(n)
    for i in range(n):
        lo = min(window, i)
        row = np.concatenate([T[i, : min(window, n - 1 - i) + 1], T[np.arange(i - lo, i), np.arange(lo, 0, -1)]])
        ref[i] = math.fsum(row)
        mag[i] = math.fsum(np.abs(row))
    return ref, mag


@pytest.mark.parametrize("snps,indiv", SHAPES)
def test_scores_within_the_summation_bound_and_reproducible(mx, monkeypatch, snps, indiv):
    X = _problem(snps, indiv, 0.05)
    ref = _restate(X, indiv)
    cp = mx.crossproduct
    import torch
    Xd = torch.from_numpy(X).to("cuda:0")
    windows = [w for w in _windows(snps) if w <= 700 or snps <= 1000]     # the fsum reference is a Python loop over snps * (2 window + 1) terms
    for window in windows:
        monkeypatch.setenv("MXA_XPROD_ENGINE", "f4")
        monkeypatch.delenv("MXA_LD_PAIRWISE_SCRATCH_MB", raising=False)
        B = cp.ld_band_pairwise(X, snps, indiv, window)
        Nband = _band_of(ref["N"], window, fill=3)
        for adjust in (False, True):
            got = {}
            for engine in ("f4", "i8"):
                monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
                for cap in (None, "2"):                                   # one group / several groups of tile rows (2 MiB: one tile row per group)
                    if cap is None:
                        monkeypatch.delenv("MXA_LD_PAIRWISE_SCRATCH_MB", raising=False)
                    else:
                        monkeypatch.setenv("MXA_LD_PAIRWISE_SCRATCH_MB", cap)
                    a = cp.ld_scores_pairwise(X, snps, indiv, window, adjust=adjust)
                    b = cp.ld_scores_pairwise(X, snps, indiv, window, adjust=adjust)
                    assert isinstance(a, np.ndarray) and a.shape == (snps,)
                    assert np.array_equal(a, b), (engine, cap, window, adjust)                 # run to run
                    got[engine, cap] = a
            monkeypatch.delenv("MXA_LD_PAIRWISE_SCRATCH_MB", raising=False)
            for key, a in got.items():
                assert np.array_equal(a, got["f4", None]), (key, window, adjust)               # engines, scratch caps
            d = cp.ld_scores_pairwise(Xd, snps, indiv, window, adjust=adjust)
            assert d.is_cuda and np.array_equal(d.cpu().numpy(), got["f4", None]), (window, adjust)   # device pointers
            want, mag = _scores_ref(B, Nband, window, adjust)
            m = 2 * window + 1
            err = np.abs(got["f4", None] - want)
            print(f"scores {snps}x{indiv} adjust={adjust} window={window}: worst |err| / bound = {float((err / (m * U * mag)).max()):.3f}")
            assert np.all(err <= m * U * mag), (window, adjust, float((err / (m * U * mag)).max()))
            if window == 0:
                assert np.array_equal(got["f4", None], _terms(B, Nband, adjust)[:, 0]), adjust      # exactly t(r_ii)


# ------------------------------------------------------------------------------------------------------ 4. chunking and the fast path
def test_band_does_not_depend_on_the_scratch_cap(mx, monkeypatch):
    snps, indiv, window = 5000, 257, 700
    from miraculix_amd.crossproduct import ld_pairwise_group_rows, ld_pairwise_tiles
    assert len(ld_pairwise_tiles(snps, window, ld_pairwise_group_rows(snps, window, scratch_mb=12))) >= 3
    X = _problem(snps, indiv, 0.05)
    for engine in ("f4", "i8"):
        monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
        monkeypatch.delenv("MXA_LD_PAIRWISE_SCRATCH_MB", raising=False)
        want = mx.crossproduct.ld_band_pairwise(X, snps, indiv, window)
        for cap in ("12", "1", "40"):
            monkeypatch.setenv("MXA_LD_PAIRWISE_SCRATCH_MB", cap)
            assert np.array_equal(mx.crossproduct.ld_band_pairwise(X, snps, indiv, window), want), (engine, cap)


@pytest.mark.parametrize("snps,indiv", SHAPES)
def test_missing_free_input_takes_the_fast_path_with_the_same_bits(mx, monkeypatch, snps, indiv):
    X = _problem(snps, indiv, 0.0)
    assert not (_codes(X, indiv) == 1).any()
    ref = _restate(X, indiv)
    window = min(700, snps - 1)
    for engine in ("f4", "i8"):
        monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
        monkeypatch.delenv("MXA_LD_PAIRWISE_DENSE", raising=False)
        rc, B = _call_band(mx, X, snps, indiv, window, window + 4, 0, False)
        assert rc == 0
        _assert_band(B, ref["r"], window, f"missing-free {snps}x{indiv} {engine}")
        S = [mx.crossproduct.ld_scores_pairwise(X, snps, indiv, window, adjust=adj) for adj in (False, True)]
        monkeypatch.setenv("MXA_LD_PAIRWISE_DENSE", "1")
        rc, B6 = _call_band(mx, X, snps, indiv, window, window + 4, 0, False)
        assert rc == 0 and np.array_equal(B6, B), engine
        for adj in (False, True):
            assert np.array_equal(mx.crossproduct.ld_scores_pairwise(X, snps, indiv, window, adjust=adj), S[adj]), (engine, adj)


# ------------------------------------------------------------------------------------------- 5. agreement with mxa_ld_band where both are defined
@pytest.mark.parametrize("snps,indiv", SHAPES)
def test_agrees_with_mxa_ld_band_on_missing_free_input(mx, snps, indiv):
    """f = the sample frequencies.  |r_pw - r_ld| <= 6 * 2^-53 * (1 + (Sxy + 4 indiv f_i f_j) / (sigma_i sigma_j)): mxa_ld's map subtracts 4 indiv f_i f_j from Sxy and
    scales by 1 / sigma, so its roundings act on terms of that size"""
    X = _problem(snps, indiv, 0.0)
    C = _codes(X, indiv)
    Z = np.where(C >= 2, C - 1, 0).astype(np.float64)
    f = Z.mean(axis=1) / 2.0
    Sxy = Z @ Z.T
    sigma = np.sqrt(np.diag(Sxy) - 4.0 * indiv * f * f)
    bound = 6 * U * (1.0 + (Sxy + 4.0 * indiv * np.outer(f, f)) / np.outer(sigma, sigma))
    for window in sorted({min(700, snps - 1), snps - 1}):
        pw = mx.crossproduct.ld_band_pairwise(X, snps, indiv, window)
        ld = mx.crossproduct.ld_band(X, snps, indiv, window, is_plink_format=True, allele_freq=f)
        inband = (np.arange(snps)[:, None] + np.arange(window + 1)[None, :]) < snps
        diff, bnd = np.abs(pw - ld)[inband], _band_of(bound, window)[inband]
        print(f"pairwise vs mxa_ld_band {snps}x{indiv} window={window}: worst |diff| / unit = {float((diff / bnd).max() * 6):.2f}")
        assert np.isfinite(pw).all() and np.all(diff <= bnd), window


# ----------------------------------------------------------------------------------------------------------------------------- 6. arguments
def test_bad_arguments_return_one_and_leave_the_output_untouched(mx):
    snps, indiv = 300, 40
    X = _problem(snps, indiv, 0.1)
    L = mx.lib.check_library_handle()
    p = mx.lib.ptr

    def band(window, ldb, kind, nind=indiv, Xs=X):
        B = np.full((snps, max(1, ldb)), SENTINEL)
        rc = L.mxa_ld_band_pairwise(p(Xs), snps, nind, window, p(B), ldb, kind)
        return rc, L.mxa_last_error(), bool(np.all(B == SENTINEL))

    def scores(window, adjust, nind=indiv, Xs=X):
        S = np.full(snps, SENTINEL)
        rc = L.mxa_ld_scores_pairwise(p(Xs), snps, nind, window, p(S), adjust)
        return rc, L.mxa_last_error(), bool(np.all(S == SENTINEL))

    bad = (1, 1, True)
    assert band(-1, 8, 0) == bad
    assert band(snps, snps + 1, 0) == bad
    assert band(10, 10, 0) == bad                      # ldb < window + 1
    assert band(10, 11, 2) == bad and band(10, 11, -1) == bad
    assert band(10, 11, 0, Xs=None) == bad
    assert band(10, 11, 0, nind=0) == bad
    assert band(10, 11, 0, nind=47_453_133) == bad     # 4 indiv^2 >= 2^53: refused before anything is read
    assert scores(-1, 0) == bad
    assert scores(snps, 0) == bad
    assert scores(10, 2) == bad
    X2 = np.ascontiguousarray(X[:, :1])                # 2 individuals: one byte per SNP
    assert scores(10, 1, nind=2, Xs=X2) == bad         # the adjusted estimator needs indiv >= 3
    assert scores(10, 0, nind=2, Xs=X2)[:2] == (0, 0)
    # the process is alive and the next good call succeeds
    assert band(10, 11, 0) == (0, 0, False)
    with pytest.raises(ValueError):
        mx.crossproduct.ld_band_pairwise(X, snps, indiv, snps)
    with pytest.raises(ValueError):
        mx.crossproduct.ld_band_pairwise(X, snps, indiv, 3, kind="r3")
    with pytest.raises(ValueError):
        mx.crossproduct.ld_scores_pairwise(X2, snps, 2, 3, adjust=True)


# ------------------------------------------------------------------------------------------------------ the gang form of the kernels
def test_band_and_scores_do_not_depend_on_the_kernel_form():
    """As test_ld_band_gpu.py does for the plain entries: MXA_XPROD_GANG=2 forces the gang-synchronised persistent kernel wherever a group's product list is long
    enough for the per-XCD lists (30 000 SNPs, window 1023: 580 band tiles, 3480 products), also with the XCD id masked so that lists are stolen -- the gang kernel
    has to hand the scratch slot of a tile entry through.  Band and scores are the same bits in all three forms and on both engines, with and without missing
    codes.  The knobs are read once per process: a child process per setting."""
    import os
    import subprocess
    import sys
    code = """
import sys, os, hashlib, numpy as np, torch
sys.path.insert(0, %r)
import miraculix_amd as mx
mx.load_shared_library()
dev = torch.device("cuda", 0)
snps, indiv, window = 30000, 300, 1023
rng = np.random.default_rng(4)
p = rng.uniform(0.1, 0.6, size=snps)
Z = rng.binomial(2, p[:, None], size=(snps, indiv)).astype(np.uint8)
h = []
for frac in (0.05, 0.0):
    code = np.where(Z == 0, 0, Z + 1).astype(np.uint8)
    code[rng.random((snps, indiv)) < frac] = 1
    code = code.reshape(snps, -1, 4)
    X = torch.from_numpy(np.ascontiguousarray(code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6))).to(dev)
    cp = mx.crossproduct
    per_engine = []
    for eng in ("f4", "i8"):
        os.environ["MXA_XPROD_ENGINE"] = eng
        B = cp.ld_band_pairwise(X, snps, indiv, window)
        inband = (torch.arange(snps, device=dev)[:, None] + torch.arange(window + 1, device=dev)[None, :]) < snps
        assert bool(torch.isfinite(B[inband]).all()) and float(B[:, 0].min()) == 1.0 and float(B[:, 0].max()) == 1.0
        S = [cp.ld_scores_pairwise(X, snps, indiv, window, adjust=a) for a in (False, True)]
        per_engine.append([hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in (B, S[0], S[1])])
    assert per_engine[0] == per_engine[1], "FP4 and int8 differ"
    h += per_engine[0]
print("hashes", *h)
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),)
    seen = set()
    for env in ({"MXA_XPROD_GANG": "0"}, {"MXA_XPROD_GANG": "2"}, {"MXA_XPROD_GANG": "2", "MXA_XPROD_GANG_XCC_MASK": "1"}):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("hashes ")]
        assert r.returncode == 0 and len(lines) == 1, (env, r.stdout + r.stderr)
        seen.add(lines[0])
    assert len(seen) == 1, seen
