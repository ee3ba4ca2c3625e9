"""Windowed LD: mxa_ld_band (the band |i - j| <= window of mxa_ld's R as LAPACK lower band storage) and mxa_ld_scores (its row sums of r^2, never
written as a matrix).  The band must equal mxa_ld's R BIT FOR BIT -- same staging, statistics, map and engines, only another tile plan and another
store -- at the shapes of test_grm_ld_fused_gpu.py, for both engines, PLINK and raw 2-bit input, host and device pointers, windows at and around the
256-SNP tile edge, with the caller's rows beyond the window untouched.  The scores are compared with math.fsum of the terms t(r), r taken from mxa_ld
of the same arguments, under the bound of ANY summation order of m = 2 window + 1 terms: |err| <= (m - 1) u sum|t| for the order plus u |l| for fsum's
one rounding, together <= m 2^-53 sum|t|; they must be identical from run to run and between the engines (fixed-order sums, no atomics)."""
import math

import numpy as np
import pytest

from _util import make_problem, pack_plink

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SHAPES = [(3000, 400), (777, 515), (130, 1031), (5000, 257)]
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


def _windows(snps):
    return sorted({w for w in (0, 1, 255, 256, 257, 700, snps - 1) if w < snps})


def _pack_raw(V):
    """V (rows x k, values 0..3) -> raw 2-bit rows, 4 fields per byte, low bits first"""
    rows, k = V.shape
    Vp = np.zeros((rows, (k + 3) // 4 * 4), dtype=np.uint8)
    Vp[:, :k] = V
    return np.ascontiguousarray((Vp[:, 0::4] | (Vp[:, 1::4] << 2) | (Vp[:, 2::4] << 4) | (Vp[:, 3::4] << 6)).astype(np.uint8))


def _band_of(R, window):
    """the band storage of the full matrix: out[i, d] = R[i, i + d], 0.0 where i + d >= snps"""
    n = R.shape[0]
    idx = np.arange(n)[:, None] + np.arange(window + 1)[None, :]
    return np.where(idx < n, R[np.arange(n)[:, None], np.minimum(idx, n - 1)], 0.0)


def _ld_map(M, f, indiv):
    """crossproduct.jl:139-149 on a given crossproduct M (as in test_grm_ld_fused_gpu.py)"""
    M = M - 4.0 * indiv * np.outer(f, f)
    s = np.sqrt(np.diag(M))
    return M / s[:, None] / s[None, :]


def _inputs(prob, fmt):
    """(packed SNP-major matrix, is_plink_format) of a problem without missing codes"""
    if fmt == "plink":
        return prob["plink"], True
    return _pack_raw(np.ascontiguousarray(prob["Z"].T).astype(np.uint8)), False


def _call_band(mx, X, snps, indiv, window, ldb, kind, is_plink, f, device):
    """the C entry with a band of leading dimension ldb pre-filled with a sentinel; returns (rc, band as a numpy (snps, ldb) array)"""
    L = mx.lib.check_library_handle()
    if device:
        import torch
        dev = torch.device("cuda", 0)
        Xd, fd = torch.from_numpy(X).to(dev), (None if f is None else torch.from_numpy(f).to(dev))
        B = torch.full((snps, ldb), SENTINEL, dtype=torch.float64, device=dev)
        rc = L.mxa_ld_band(mx.lib.ptr(Xd), snps, indiv, window, mx.lib.ptr(B), ldb, kind, int(is_plink), mx.lib.ptr(fd))
        torch.cuda.synchronize()
        return rc, B.cpu().numpy()
    B = np.full((snps, ldb), SENTINEL, dtype=np.float64)
    rc = L.mxa_ld_band(mx.lib.ptr(X), snps, indiv, window, mx.lib.ptr(B), ldb, kind, int(is_plink), mx.lib.ptr(f))
    return rc, B


def _check_band_against_full(mx, X, snps, indiv, is_plink, f, device, equal_nan=False):
    """every window, both kinds: the band equals the band of mxa_ld's R bit for bit, exact zeros in the tail, the sentinel beyond the window"""
    R = mx.crossproduct.ld(X, snps, indiv, is_plink_format=is_plink, allele_freq=f)
    for window in _windows(snps):
        ldb = window + 4
        want = _band_of(R, window)
        for kind in (0, 1):
            rc, B = _call_band(mx, X, snps, indiv, window, ldb, kind, is_plink, f, device)
            assert rc == 0, (window, kind, mx.lib.last_error())
            assert np.array_equal(B[:, : window + 1], want * want if kind else want, equal_nan=equal_nan), (window, kind)
            tail = (np.arange(snps)[:, None] + np.arange(window + 1)[None, :]) >= snps
            assert np.all(B[:, : window + 1][tail] == 0.0) and not np.signbit(B[:, : window + 1][tail]).any(), (window, kind)
            assert np.all(B[:, window + 1:] == SENTINEL), (window, kind)
    return R


@pytest.mark.parametrize("snps,indiv", SHAPES)
@pytest.mark.parametrize("engine", ["f4", "i8"])
@pytest.mark.parametrize("fmt", ["plink", "raw"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_band_equals_the_band_of_mxa_ld_bit_for_bit(mx, monkeypatch, snps, indiv, engine, fmt, device):
    monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
    prob = make_problem(snps, indiv, 1, seed=snps + indiv)
    X, is_plink = _inputs(prob, fmt)
    R = _check_band_against_full(mx, X, snps, indiv, is_plink, prob["f"], device)
    assert np.isfinite(R).all()                    # no monomorphic SNP at these shapes: nothing is excluded above
    # the Python binding: shape (snps, window + 1), numpy in -> numpy out, device tensor in -> device tensor out
    w = min(257, snps - 1)
    if device:
        import torch
        dev = torch.device("cuda", 0)
        B = mx.crossproduct.ld_band(torch.from_numpy(X).to(dev), snps, indiv, w, kind="r2", is_plink_format=is_plink, allele_freq=torch.from_numpy(prob["f"]).to(dev))
        assert B.is_cuda and tuple(B.shape) == (snps, w + 1)
        B = B.cpu().numpy()
    else:
        B = mx.crossproduct.ld_band(X, snps, indiv, w, kind="r2", is_plink_format=is_plink, allele_freq=prob["f"])
        assert isinstance(B, np.ndarray) and B.shape == (snps, w + 1)
    want = _band_of(R, w)
    assert np.array_equal(B, want * want)


@pytest.mark.parametrize("engine", ["f4", "i8"])
def test_band_with_missing_codes_under_the_plink_byte_table(mx, monkeypatch, engine):
    """a byte that holds a missing pair is staged as 0xFF (four 3s), exactly as mxa_ld stages it"""
    monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
    snps, indiv = 777, 515
    prob = make_problem(snps, indiv, 1, seed=5, missing_frac=0.05)
    assert ((prob["plink"] & 0x55) & ~((prob["plink"] >> 1) & 0x55)).any()     # missing pairs (01) are there
    _check_band_against_full(mx, prob["plink"], snps, indiv, True, prob["f"], device=False, equal_nan=True)


def test_band_and_scores_with_a_monomorphic_snp_are_non_finite_as_mxa_ld_is(mx):
    """sigma = 0: mxa_ld gives non-finite entries in that SNP's row and column; the band gives the same ones, a score whose window holds one is
    non-finite, every other score is unaffected -- no special case anywhere"""
    snps, indiv = 777, 515
    prob = make_problem(snps, indiv, 1, seed=6)
    Z = prob["Z"].copy()
    mono = 256                                         # first SNP of the second tile
    Z[:, mono] = 0
    X = pack_plink(np.ascontiguousarray(Z.T))
    f = Z.astype(np.float64).mean(axis=0) / 2.0
    R = _check_band_against_full(mx, X, snps, indiv, True, f, device=False, equal_nan=True)
    assert not np.isfinite(R[mono]).any() and np.isfinite(np.delete(np.delete(R, mono, 0), mono, 1)).all()
    w = 100
    S = mx.crossproduct.ld_scores(X, snps, indiv, w, is_plink_format=True, allele_freq=f)
    near = np.abs(np.arange(snps) - mono) <= w
    assert not np.isfinite(S[near]).any() and np.isfinite(S[~near]).all()


# ------------------------------------------------------------------------------------------------------------- planted LD
def _planted_problem(snps, indiv, seed):
    """blocks of four SNPs: SNP 4b is drawn as in make_problem, SNPs 4b + 1 .. 4b + 3 are copies of it in which 10 % of the individuals are redrawn --
    large r at the offsets 1..3 inside a block, near 0 elsewhere, so a wrong diagonal offset cannot hide in noise"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.6, size=snps)
    Z = rng.binomial(2, p[None, :], size=(indiv, snps)).astype(np.int8)
    for q in range(1, 4):
        cols = np.arange(q, snps, 4)
        keep = rng.random((indiv, len(cols))) >= 0.1
        Z[:, cols] = np.where(keep, Z[:, cols - q], rng.binomial(2, p[cols - q][None, :], size=(indiv, len(cols))))
    return dict(Z=Z, plink=np.ascontiguousarray(pack_plink(np.ascontiguousarray(Z.T))), f=Z.astype(np.float64).mean(axis=0) / 2.0)


@pytest.mark.parametrize("snps,indiv", SHAPES)
@pytest.mark.parametrize("engine", ["f4", "i8"])
def test_band_on_planted_ld_against_mxa_ld_and_the_dense_restatement(mx, monkeypatch, snps, indiv, engine):
    monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
    prob = _planted_problem(snps, indiv, seed=3 * snps + indiv)
    Zf = prob["Z"].astype(np.float64)
    ref = _ld_map(Zf.T @ Zf, prob["f"], indiv)
    assert np.isfinite(ref).all()
    assert np.abs(np.diagonal(ref, 1)[0::4]).min() > 0.5 and np.abs(np.diagonal(ref, 4)).max() < 0.5    # the planted structure is there
    _check_band_against_full(mx, prob["plink"], snps, indiv, True, prob["f"], device=False)
    for window in _windows(snps):
        B = mx.crossproduct.ld_band(prob["plink"], snps, indiv, window, is_plink_format=True, allele_freq=prob["f"])
        want = _band_of(ref, window)
        assert np.abs(B - want).max() <= 1e-12 * np.abs(ref).max(), window     # the tolerance test_grm_ld_fused_gpu.py states for mxa_ld


# ------------------------------------------------------------------------------------------------------------------- scores
def _terms(R, indiv, adjust):
    """t(r) with the kernel's operation order, every operation rounded on its own: r2 = r * r; adjusted: r2 - (1 - r2) * (1 / (indiv - 2))"""
    r2 = R * R
    if not adjust:
        return r2
    inv = 1.0 / (float(indiv) - 2.0)
    return r2 - (1.0 - r2) * inv


def _scores_ref(T, window):
    """per SNP: fsum of the terms within the window, and sum|t|"""
    n = T.shape[0]
    ref, mag = np.empty(n), np.empty(n)
    for i in range(n):
        row = T[i, max(0, i - window): min(n, i + window + 1)]
        ref[i] = math.fsum(row)
        mag[i] = math.fsum(np.abs(row))
    return ref, mag


@pytest.mark.parametrize("snps,indiv", SHAPES)
@pytest.mark.parametrize("fmt", ["plink", "raw", "planted"])
def test_scores_within_the_summation_bound_and_reproducible_across_runs_and_engines(mx, monkeypatch, snps, indiv, fmt):
    if fmt == "planted":
        prob = _planted_problem(snps, indiv, seed=3 * snps + indiv)
        X, is_plink = prob["plink"], True
    else:
        prob = make_problem(snps, indiv, 1, seed=snps + indiv)
        X, is_plink = _inputs(prob, fmt)
    f = prob["f"]
    cp = mx.crossproduct
    monkeypatch.setenv("MXA_XPROD_ENGINE", "f4")
    R = cp.ld(X, snps, indiv, is_plink_format=is_plink, allele_freq=f)
    assert np.isfinite(R).all()
    import torch
    dev = torch.device("cuda", 0)
    Xd, fd = torch.from_numpy(X).to(dev), torch.from_numpy(f).to(dev)
    for adjust in (False, True):
        T = _terms(R, indiv, adjust)
        for window in _windows(snps):
            got = {}
            for engine in ("f4", "i8"):
                monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
                a = cp.ld_scores(X, snps, indiv, window, adjust=adjust, is_plink_format=is_plink, allele_freq=f)
                b = cp.ld_scores(X, snps, indiv, window, adjust=adjust, is_plink_format=is_plink, allele_freq=f)
                assert isinstance(a, np.ndarray) and a.shape == (snps,)
                assert np.array_equal(a, b), (engine, window, adjust)                     # run to run
                got[engine] = a
            assert np.array_equal(got["f4"], got["i8"]), (window, adjust)                 # engine to engine
            d = cp.ld_scores(Xd, snps, indiv, window, adjust=adjust, is_plink_format=is_plink, allele_freq=fd)
            assert d.is_cuda and np.array_equal(d.cpu().numpy(), got["i8"]), (window, adjust)   # device pointers
            ref, mag = _scores_ref(T, window)
            m = 2 * window + 1
            err = np.abs(got["f4"] - ref)
            print(f"scores {snps}x{indiv} {fmt} adjust={adjust} window={window}: worst |err| / bound = {float((err / (m * U * mag)).max()):.3f}")
            assert np.all(err <= m * U * mag), (window, adjust, float((err / (m * U * mag)).max()))
            if window == 0:
                assert np.array_equal(got["f4"], np.diagonal(T)), adjust                  # exactly t(R_ii)


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_bad_arguments_return_one_and_leave_the_output_untouched(mx):
    snps, indiv = 300, 40
    prob = make_problem(snps, indiv, 1, seed=9)
    X, f = prob["plink"], prob["f"]
    L = mx.lib.check_library_handle()
    p = mx.lib.ptr

    def band(window, ldb, kind, freq, nind=indiv):
        B = np.full((snps, max(1, ldb)), SENTINEL)
        rc = L.mxa_ld_band(p(X), snps, nind, window, p(B), ldb, kind, 1, p(freq))
        return rc, L.mxa_last_error(), bool(np.all(B == SENTINEL))

    def scores(window, adjust, freq, nind=indiv, Xs=X):
        S = np.full(snps, SENTINEL)
        rc = L.mxa_ld_scores(p(Xs), snps, nind, window, p(S), adjust, 1, p(freq))
        return rc, L.mxa_last_error(), bool(np.all(S == SENTINEL))

    bad = (1, 1, True)
    assert band(-1, 8, 0, f) == bad
    assert band(snps, snps + 1, 0, f) == bad
    assert band(10, 10, 0, f) == bad                   # ldb < window + 1
    assert band(10, 11, 2, f) == bad and band(10, 11, -1, f) == bad
    assert band(10, 11, 0, None) == bad
    assert scores(-1, 0, f) == bad
    assert scores(snps, 0, f) == bad
    assert scores(10, 0, None) == bad
    X2 = np.ascontiguousarray(X[:, :1])                # 2 individuals: one byte per SNP
    assert scores(10, 1, f, nind=2, Xs=X2) == bad      # the adjusted estimator divides by indiv - 2
    assert scores(10, 0, f, nind=2, Xs=X2)[:2] == (0, 0)
    # the process is alive and the next good call succeeds
    rc, err, untouched = band(10, 11, 0, f)
    assert (rc, err, untouched) == (0, 0, False)
    with pytest.raises(ValueError):
        mx.crossproduct.ld_band(X, snps, indiv, snps, is_plink_format=True, allele_freq=f)
    with pytest.raises(ValueError):
        mx.crossproduct.ld_band(X, snps, indiv, 3, kind="r3", is_plink_format=True, allele_freq=f)
    with pytest.raises(ValueError):
        mx.crossproduct.ld_scores(X, snps, indiv, 3, is_plink_format=True, allele_freq=None)


# ------------------------------------------------------------------------------------------------------ the gang form of the kernels
def test_band_and_scores_do_not_depend_on_the_kernel_form():
    """The launch takes the gang-synchronised persistent kernel only for long tiles (K >= 131k), which no small test reaches by itself: MXA_XPROD_GANG=2
    forces it wherever the tile list is long enough for the per-XCD lists (30 000 SNPs, window 1023: 580 tiles), also with the XCD id masked so that lists
    are stolen.  In every form the band equals mxa_ld's band bit for bit, and the scores are the same bits in all three forms and on both engines.  The knobs
    are read once per process: a child process per setting."""
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
code = np.where(Z == 0, 0, Z + 1).astype(np.uint8).reshape(snps, -1, 4)
X = torch.from_numpy(np.ascontiguousarray(code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6))).to(dev)
f = torch.from_numpy(Z.astype(np.float64).mean(axis=1) / 2.0).to(dev)
cp = mx.crossproduct
R = cp.ld(X, snps, indiv, is_plink_format=True, allele_freq=f)
idx = torch.arange(snps, device=dev)[:, None] + torch.arange(window + 1, device=dev)[None, :]
want = torch.where(idx < snps, R[torch.arange(snps, device=dev)[:, None], idx.clamp(max=snps - 1)], torch.zeros((), dtype=torch.float64, device=dev))
del R
h = []
for eng in ("f4", "i8"):
    os.environ["MXA_XPROD_ENGINE"] = eng
    B = cp.ld_band(X, snps, indiv, window, is_plink_format=True, allele_freq=f)
    assert torch.equal(B, want), eng
    for adjust in (False, True):
        S = cp.ld_scores(X, snps, indiv, window, adjust=adjust, is_plink_format=True, allele_freq=f)
        assert bool(torch.isfinite(S).all())
        h.append(hashlib.sha256(S.cpu().numpy().tobytes()).hexdigest())
assert h[0] == h[2] and h[1] == h[3], "FP4 and int8 scores differ"
print("scores", h[0], h[1])
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),)
    seen = set()
    for env in ({"MXA_XPROD_GANG": "0"}, {"MXA_XPROD_GANG": "2"}, {"MXA_XPROD_GANG": "2", "MXA_XPROD_GANG_XCC_MASK": "1"}):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("scores ")]
        assert r.returncode == 0 and len(lines) == 1, (env, r.stdout + r.stderr)
        seen.add(lines[0])
    assert len(seen) == 1, seen
