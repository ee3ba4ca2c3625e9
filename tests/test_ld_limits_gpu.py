"""The LD pairs, prune, apply and operator entries (mxa_ld_window_pairs, mxa_ld_prune_csr, mxa_ld_window_apply*, mxa_ld_op_*) at their limits.

  A. block and chunk edges, small and exact: the operator at snps in {1, 2, 255 .. 257, 1023 .. 1025, 2049} (kOpRows = 256, kDotRows = 1024) and every chunk
     width of k_ld_op_apply<NC, U> (n = 1 .. 33: <2, 8>, a full <4, 4>, partial <8, 4> and <16, 4>); the solve there, a column against its one-column solve;
     65 535 columns of a solve (gridDim.y) and 1 048 560 columns of mxa_ld_window_apply, and one more of each rejected; mxa_ld_window_apply(_pairwise) at tiny
     and ragged shapes with the references and bounds of tests/test_ld_apply_gpu.py;
  B. launches of 2^32 threads and more: the operator at 2^24 + 300 SNPs (one workgroup of 256 per SNP), mxa_ld_prune_csr at 2^26 + 5 SNPs (a wave per SNP);
  C. more than 2^31 stored entries: the operator's mirrored array (4.5 10^9 doubles), the CSR of the pairs entry and the prune on it, the apply's partial sums.

The closed forms are in tests/_ld_limits_ref.py (held to the brute-force helpers by tests/test_ld_limits_cpu.py); everything but one check is equality.  The one
bound: the ones column of mxa_ld_window_apply at term 1 against mxa_ld_window_scores within 2 m u sum|t| (test_ld_apply_gpu.py's, the same terms in two
orders).  Large operands are built on the device; a test that needs more free device memory than there is skips (an MI355X runs them all)."""
import ctypes
import time

import numpy as np
import pytest

import _ld_apply_ref as ar
import _ld_limits_ref as lim
import _ld_op_ref as opr
import _ld_ref as ref
import test_ld_apply_gpu as tap
from _util import pack_plink
from test_ld_op_gpu import SHIFTS, TOL, _bits, _from_rows
from test_ld_window_edges_gpu import _edge_case

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SENTINEL = -12345.678
SENT_I, SENT_B, SENT_L = -777_777, 0xAB, -7_777_777_777
PAD = 67
EDGE_SNPS = (1, 2, 255, 256, 257, 1023, 1024, 1025, 2049)
EDGE_NS = (1, 2, 4, 5, 7, 8, 9, 15, 16, 31, 32, 33)
APPLY_SHAPES = [(1, 5), (2, 6), (255, 6), (256, 70), (257, 6), (513, 70)]


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


@pytest.fixture(autouse=True)
def _default_environment(monkeypatch):
    monkeypatch.delenv("MXA_XPROD_ENGINE", raising=False)
    monkeypatch.delenv("MXA_LD_PAIRWISE_SCRATCH_MB", raising=False)
    monkeypatch.delenv("MXA_LD_PAIRWISE_DENSE", raising=False)


def _need(gb):
    import torch
    if torch.cuda.mem_get_info()[0] < gb * 10 ** 9:
        pytest.skip(f"needs {gb} GB of free device memory")
    return torch.device("cuda", 0)


def _differ(got, want):
    """'' when the tensors are equal, else how many elements differ and where the first ones are (the assertion's message)"""
    import torch
    if torch.equal(got, want):
        return ""
    bad = torch.nonzero((got != want).reshape(-1))[:, 0]
    return f"{bad.numel()} of {want.numel()} differ, first at {bad[:4].tolist()}, last at {int(bad[-1])}"


def _edge_windows(snps):
    """w = 0, 1 and snps - 1, and the seeded geometries 0 .. 2 of _ld_ref.sweep_window where they are defined (chromosome ends at 32 k + o: snps > 32)"""
    out = [(f"w={w}", ref.fixed_last(snps, w)) for w in sorted({0, 1, snps - 1}) if w < snps]
    if snps > 32:
        out += [(f"sweep {s}", ref.sweep_window(snps, s)) for s in range(3)]
    return out


# ------------------------------------------------------------------------------------------------------------------- A1. operator, exact
@pytest.mark.parametrize("snps", EDGE_SNPS)
def test_operator_at_block_and_chunk_edges_bit_for_bit(mx, snps):
    Xi = np.random.default_rng([snps, 1]).integers(-4, 5, (snps, max(EDGE_NS))).astype(np.float64)
    for name, last in _edge_windows(snps):
        rows = opr.dyadic_rows(last)
        W = opr.windowed(ar.dense(rows, last), last)
        with _from_rows(mx, last, rows) as op:
            assert np.array_equal(_bits(op.rows()), _bits(rows)), name
            assert np.array_equal(_bits(op.rows(device=True)), _bits(rows)), name
            for shift in SHIFTS:
                want = opr.apply_exact(W, Xi, shift)
                for n in EDGE_NS:
                    Y = op.apply(Xi[:, :n], shift, device=n in (5, 33))          # Op.apply asserts the sentinel rows and the guard column
                    assert np.array_equal(Y, want[:, :n]), (name, shift, n, np.argwhere(Y != want[:, :n])[:3])


# -------------------------------------------------------------------------------------------------------------------------- A2. solve
@pytest.mark.parametrize("snps", EDGE_SNPS)
def test_solve_at_block_edges_and_a_column_is_its_one_column_solve(mx, snps):
    B = np.random.default_rng([snps, 2]).standard_normal((snps, 33))
    for name, last in _edge_windows(snps):
        rows = opr.decay_rows(last)
        W = opr.windowed(ar.dense(rows, last), last)
        with _from_rows(mx, last, rows) as op:
            X33, it33, rel33, st33 = op.solve(B, 1.5)
            assert np.all(st33 == 0) and np.all(rel33 <= TOL), (name, st33, rel33.max())
            true = opr.true_relres(W, 1.5, X33, B)
            assert np.all(true <= 2 * TOL), (name, float(true.max()))
            X9, it9, rel9, st9 = op.solve(B[:, :9], 1.5, device=True)
            for c in range(33):
                x1, it1, rel1, st1 = op.solve(B[:, c: c + 1], 1.5)
                for n, (Xn, itn, reln, stn) in ((33, (X33, it33, rel33, st33)), (9, (X9, it9, rel9, st9))):
                    if c < n:
                        assert np.array_equal(_bits(x1[:, 0]), _bits(Xn[:, c])), (name, n, c)
                        assert (it1[0], st1[0]) == (itn[c], stn[c]) and _bits(rel1)[0] == _bits(reln)[c], (name, n, c)


# ------------------------------------------------------------------------------------------------------------ A3. columns at the grid limits
def test_solve_with_65535_columns_and_one_more_rejected(mx):
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    snps, n, zero = 257, 65535, 7
    SHIFT = 4.0                                              # 5 on the diagonal, at most 1 off it: ten iterations, each three one-workgroup passes over the columns
    last = ref.fixed_last(snps, 1)
    B = np.random.default_rng([snps, 3]).standard_normal((snps, n))
    B[:, zero] = 0.0
    with _from_rows(mx, last, opr.decay_rows(last)) as op:
        t0 = time.perf_counter()
        X, iters, relres, status = op.solve(B, SHIFT, device=True)
        print(f"ld_op solve {snps} x {n}: {time.perf_counter() - t0:.2f} s, iters {iters.min()} .. {iters.max()}")
        assert np.all(status == 0) and np.all(relres <= TOL)
        assert iters[zero] == 0 and relres[zero] == 0.0 and np.all(X[:, zero] == 0.0)
        for c in (0, n - 1, zero):
            x1, it1, rel1, st1 = op.solve(B[:, c: c + 1], SHIFT)
            assert np.array_equal(_bits(x1[:, 0]), _bits(X[:, c])), c
            assert (it1[0], st1[0]) == (iters[c], status[c]) and _bits(rel1)[0] == _bits(relres)[c], c
        del X
        n1 = n + 1
        Bp, Xs = np.ones((n1, snps)), np.full((n1 + 1, snps), SENTINEL)
        it, rel, st = np.full(n1, -7, np.int32), np.full(n1, SENTINEL), np.full(n1, -7, np.int32)
        rc = L.mxa_ld_op_solve(op.h, SHIFT, p(Bp), snps, n1, p(Xs), snps, TOL, 1000, p(it), p(rel), p(st))
        assert (rc, L.mxa_last_error()) == (1, 1)
        assert np.all(Xs == SENTINEL) and np.all(it == -7) and np.all(rel == SENTINEL) and np.all(st == -7)


def test_window_apply_with_1048560_columns_and_one_more_rejected(mx):
    import torch
    dev = _need(12)                                          # 4 KiB of partial sums per column and window tile: 4.3 GB
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    snps, indiv, n = 1, 6, 1_048_560
    Z = np.array([[0, 1, 2, 0, 1, 2]], np.int8)
    X, f, last = np.ascontiguousarray(pack_plink(Z)), np.array([0.5]), np.zeros(1, np.int32)
    r00 = np.full(1 + PAD, SENTINEL)
    assert L.mxa_ld_window_rows(p(X), snps, indiv, p(last), p(r00), 0, 1, p(f)) == 0, mx.lib.last_error()
    assert np.isfinite(r00[0]) and r00[0] != 0.0 and np.all(r00[1:] == SENTINEL)
    Xv = np.random.default_rng(4).standard_normal(n + 1)
    Xd = torch.from_numpy(Xv).to(dev)
    Yd = torch.full((n + 1 + PAD,), SENTINEL, dtype=torch.float64, device=dev)
    rc = L.mxa_ld_window_apply(p(X), snps, indiv, p(last), 0, p(Xd), 1, n, p(Yd), 1, 1, p(f))
    assert (rc, L.mxa_last_error()) == (0, 0), mx.lib.last_error()
    torch.cuda.synchronize()
    Y = Yd.cpu().numpy()
    assert np.all(Y[n:] == SENTINEL), "written behind column n - 1"
    assert np.array_equal(_bits(Y[:n]), _bits(r00[0] * Xv[:n]))           # one product, one rounding
    Yd.fill_(SENTINEL)
    rc = L.mxa_ld_window_apply(p(X), snps, indiv, p(last), 0, p(Xd), 1, n + 1, p(Yd), 1, 1, p(f))
    assert (rc, L.mxa_last_error()) == (1, 1) and bool((Yd == SENTINEL).all())


# ------------------------------------------------------------------------------------- A5. windowed apply at tiny and ragged sizes
def _apply_case(snps, indiv, route):
    c = _edge_case(snps, indiv)                              # every SNP polymorphic; the pairwise data: every pair shares >= 3 individuals, none constant there
    if route == "plain":
        return dict(X=c["X"], f=c["f"], N=None)
    return dict(X=c["Xp"], f=None, N=ar.present_counts(c["Xp"], indiv))


def _apply_windows(snps):
    out = [(f"w={w}", ref.fixed_last(snps, w)) for w in sorted({0, 1, snps - 1}) if w < snps]
    if snps >= 2:
        cut = snps // 2
        out.append(("two chromosomes", np.where(np.arange(snps) < cut, cut - 1, snps - 1).astype(np.int32)))
    return out


@pytest.mark.parametrize("route", ("plain", "pairwise-missing"))
@pytest.mark.parametrize("snps,indiv", APPLY_SHAPES)
def test_window_apply_at_tiny_and_ragged_sizes(mx, snps, indiv, route):
    case = _apply_case(snps, indiv, route)
    Xm = tap._x(snps)
    units = sorted({0, snps // 2, snps - 1})
    E = np.zeros((snps, len(units)))
    E[units, np.arange(len(units))] = 1.0
    worst = 0.0
    for name, last in _apply_windows(snps):
        first = ref.first_of(last)
        R = tap._rows(mx, case, route, snps, indiv, last)
        for term in (0, 1, 2):
            T = tap._terms(R, case, route, indiv, term)
            want, mag, m = ar.apply_ref(T, last, Xm)
            assert np.isfinite(want).all()
            bound = (m[:, None] + 2.0) * U * mag
            for n in tap.NS:
                Y = tap._apply(mx, case, route, snps, indiv, last, term, Xm[:, :n], device=n == 7)
                err = np.abs(Y - want[:, :n])
                with np.errstate(invalid="ignore", divide="ignore"):
                    worst = max(worst, float(np.nanmax(np.where(err > 0, err / bound[:, :n], 0.0))))
                assert np.all(err <= bound[:, :n]), (name, term, n, worst)
            Y = tap._apply(mx, case, route, snps, indiv, last, term, E)
            for c, k in enumerate(units):
                inside = (first <= k) & (k <= last)
                assert np.array_equal(_bits(Y[inside, c]), _bits(T[inside, k])), (name, term, k)
                assert np.all(Y[~inside, c] == 0.0), (name, term, k)
    print(f"apply {route} {snps}x{indiv}: worst |err| / bound = {worst:.3f}")


# ----------------------------------------------------------------------------------------------------- B1. the operator past 2^24 SNPs
class _RawOp:
    """mxa_ld_op_* on device tensors (n x snps: column-major with ld = snps), one guard column of sentinels behind Y / X"""

    def __init__(self, mx, snps, last, rows):
        self.mx, self.snps, self.L, self.p = mx, snps, mx.lib.check_library_handle(), mx.lib.ptr
        self.h = ctypes.c_void_p(None)
        rc = self.L.mxa_ld_op_from_rows(snps, self.p(last), self.p(rows), ctypes.byref(self.h))
        assert rc == 0 and self.h.value, mx.lib.last_error()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.L.mxa_ld_op_free(ctypes.byref(self.h))
        return False

    def rows(self, entries):
        import torch
        out = torch.full((entries + PAD,), SENTINEL, dtype=torch.float64, device="cuda")
        assert self.L.mxa_ld_op_rows(self.h, self.p(out)) == 0, self.mx.lib.last_error()
        torch.cuda.synchronize()
        assert bool((out[entries:] == SENTINEL).all())
        return out[:entries]

    def apply(self, X, shift):
        import torch
        n = X.shape[0]
        Y = torch.full((n + 1, self.snps), SENTINEL, dtype=torch.float64, device="cuda")
        rc = self.L.mxa_ld_op_apply(self.h, shift, self.p(X), self.snps, n, self.p(Y), self.snps)
        assert (rc, self.L.mxa_last_error()) == (0, 0), self.mx.lib.last_error()
        torch.cuda.synchronize()
        assert bool((Y[n] == SENTINEL).all()), "written outside Y"
        return Y[:n]

    def solve(self, B, shift):
        import torch
        n = B.shape[0]
        X = torch.full((n + 1, self.snps), SENTINEL, dtype=torch.float64, device="cuda")
        iters, relres, status = np.full(n + 1, -7, np.int32), np.full(n + 1, SENTINEL), np.full(n + 1, -7, np.int32)
        rc = self.L.mxa_ld_op_solve(self.h, shift, self.p(B), self.snps, n, self.p(X), self.snps, TOL, 1000, self.p(iters), self.p(relres), self.p(status))
        assert (rc, self.L.mxa_last_error()) == (0, 0), self.mx.lib.last_error()
        torch.cuda.synchronize()
        assert bool((X[n] == SENTINEL).all()) and iters[n] == -7 and relres[n] == SENTINEL and status[n] == -7
        return X[:n], iters[:n], relres[:n], status[:n]


def test_operator_with_more_than_two_to_the_24_snps(mx):
    """k_ld_op_mirror / k_ld_op_upper run one workgroup of 256 threads per SNP: 2^32 threads from 2^24 SNPs on"""
    dev = _need(8)
    snps, w, coef = (1 << 24) + 300, 1, lim.B1_COEF
    entries, _ = lim.band_entries(snps, w)
    last, rows = lim.band_last(snps, w, dev), lim.band_rows(snps, w, coef, dev)
    with _RawOp(mx, snps, last, rows) as op:
        assert not (msg := _differ(op.rows(entries), rows)), "mxa_ld_op_rows: " + msg
        for n in (1, 3):
            X = lim.band_x(snps, n, dev)
            for shift in (0.0, 0.5):
                assert not (msg := _differ(op.apply(X, shift), lim.band_apply(snps, w, coef, X, shift))), f"apply n {n} shift {shift}: " + msg
        B = lim.band_x(snps, 2, dev)
        X, iters, relres, status = op.solve(B, 2.0)                       # 3 on the diagonal, at most 2 off it: diagonally dominant
        true = lim.relres(B, B - lim.band_apply(snps, w, coef, X, 2.0))
        print(f"ld_op solve at {snps} SNPs: iters {iters.tolist()}, relres {relres.tolist()}, true {true.tolist()}")
        assert np.all(status == 0) and np.all(relres <= TOL) and np.all(true <= 2 * TOL)


# -------------------------------------------------------------------------------------------- B2. mxa_ld_prune_csr past 2^26 SNPs
def _prune_csr(mx, snps, rowptr, col, prio, with_owner):
    """(keep, owner or None, n_kept, rounds) on device outputs with PAD sentinels behind them"""
    import torch
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    keep = torch.full((snps + PAD,), SENT_B, dtype=torch.uint8, device="cuda")
    owner = torch.full((snps + PAD,), SENT_I, dtype=torch.int32, device="cuda") if with_owner else None
    n_kept, rounds = ctypes.c_long(SENT_L), ctypes.c_int(-777)
    rc = L.mxa_ld_prune_csr(snps, p(rowptr), p(col), p(prio), p(keep), p(owner), ctypes.byref(n_kept), ctypes.byref(rounds))
    assert (rc, L.mxa_last_error()) == (0, 0), mx.lib.last_error()
    torch.cuda.synchronize()
    assert bool((keep[snps:] == SENT_B).all()) and (owner is None or bool((owner[snps:] == SENT_I).all()))
    return keep[:snps], None if owner is None else owner[:snps], n_kept.value, rounds.value


def test_prune_csr_with_more_than_two_to_the_26_snps(mx):
    """k_ld_prune_edges / k_ld_prune_owner / k_ld_prune_check_col run one wave per SNP, four per workgroup: 2^32 threads from 2^26 SNPs on"""
    import torch
    dev = _need(6)
    snps = (1 << 26) + 5
    edges = lim.b2_edges(snps)
    rowptr, col = lim.sparse_csr(snps, edges, dev)
    for reverse in (False, True):
        prio = -torch.arange(snps, dtype=torch.float64, device=dev) if reverse else None
        touched, keep_t, owner_t, want_kept = lim.sparse_prune_expected(snps, edges, reverse)
        want_keep = torch.ones(snps, dtype=torch.uint8, device=dev)
        want_owner = torch.arange(snps, dtype=torch.int32, device=dev)
        td = torch.from_numpy(touched).to(dev)
        want_keep[td] = torch.from_numpy(keep_t.astype(np.uint8)).to(dev)
        want_owner[td] = torch.from_numpy(owner_t.astype(np.int32)).to(dev)
        for with_owner in (True, False):
            keep, owner, n_kept, rounds = _prune_csr(mx, snps, rowptr, col, prio, with_owner)
            what = f"priority {'-i' if reverse else 'NULL'}, owner {with_owner}: "
            assert not (msg := _differ(keep, want_keep)), what + "keep: " + msg
            assert owner is None or not (msg := _differ(owner, want_owner)), what + "owner: " + msg
            assert n_kept == want_kept and 1 <= rounds <= snps, (what, n_kept, want_kept, rounds)
            del keep, owner
        del prio, want_keep, want_owner


# ------------------------------------------------------------------------------------ C1. the operator with 4.5 10^9 mirrored entries
def test_operator_with_more_than_two_to_the_32_mirrored_entries(mx):
    import torch
    dev = _need(80)                                          # the input rows, the upper rows and the mirrored rows: 18 + 18 + 36 GB
    snps, w, coef = 1_100_000, 2047, lim.C1_COEF
    entries, mirrored = lim.band_entries(snps, w)
    assert entries == 2_250_703_872 > 2 ** 31 and mirrored == 4_500_307_744 > 2 ** 32
    last, rows = lim.band_last(snps, w, dev), lim.band_rows(snps, w, coef, dev)
    with _RawOp(mx, snps, last, rows) as op:
        back = op.rows(entries)
        assert not (msg := _differ(back, rows)), "mxa_ld_op_rows: " + msg
        del back, rows
        torch.cuda.empty_cache()
        X = lim.band_x(snps, 3, dev)
        for shift in (0.0, 0.5):
            assert not (msg := _differ(op.apply(X, shift), lim.band_apply(snps, w, coef, X, shift))), f"apply shift {shift}: " + msg


# ----------------------------------------------------------------- C2 / C3. pairs, prune and apply on 100 000 x 64, w = 32 767
BIG_COLUMNS = (0, 50_000, 99_999)


@pytest.fixture(scope="module")
def big(mx):
    """the shared problem on the device; of its 21.9 GB of ragged rows (mxa_ld_window_rows, kind 0) the sampled positions, the window's part of the columns
    BIG_COLUMNS and the whole windows of 32 rows are kept, the buffer is freed"""
    import torch
    dev = _need(45)
    P = lim.big_window_problem()
    snps, indiv, w, total, rowptr = P["snps"], P["indiv"], P["w"], P["total"], P["rowptr"]
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    Xd, fd, lastd = torch.from_numpy(P["X"]).to(dev), torch.from_numpy(P["f"]).to(dev), torch.from_numpy(P["last"]).to(dev)
    out = torch.full((total + PAD,), SENTINEL, dtype=torch.float64, device=dev)
    assert L.mxa_ld_window_rows(p(Xd), snps, indiv, p(lastd), p(out), 0, 1, p(fd)) == 0, mx.lib.last_error()
    torch.cuda.synchronize()
    assert bool((out[total:] == SENTINEL).all())

    def window_of(k):
        """(lo, hi, flat positions of T[i, k], i = lo .. hi): the pair (min, max) lies in row min at offset max - min"""
        lo, hi = max(0, k - w), min(snps - 1, k + w)
        i = np.arange(lo, hi + 1)
        return lo, hi, np.where(i <= k, rowptr[np.minimum(i, k)] + (k - i), rowptr[k] + (i - k))

    take = lambda pos: out[torch.from_numpy(np.ascontiguousarray(pos)).to(dev)].cpu().numpy()
    sampled = take(P["k"])
    columns = {}
    for k in BIG_COLUMNS:
        lo, hi, pos = window_of(k)
        columns[k] = (lo, hi, take(pos), int(pos.max()))
    score_rows = np.concatenate([[0, snps - 1], P["rng"].integers(1, snps - 1, size=30)])
    windows = {int(i): take(window_of(int(i))[2]) for i in score_rows}
    del out
    torch.cuda.empty_cache()
    assert np.isfinite(sampled).all()
    return dict(P=P, Xd=Xd, fd=fd, lastd=lastd, sampled=sampled, columns=columns, windows=windows)


def test_pairs_then_prune_with_more_than_two_to_the_31_pairs(mx, big):
    import torch
    dev = torch.device("cuda", 0)
    P, Xd, fd, lastd = big["P"], big["Xd"], big["fd"], big["lastd"]
    snps, indiv, w = P["snps"], P["indiv"], P["w"]
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    rowptr = torch.full((snps + 1 + PAD,), SENT_L, dtype=torch.int64, device=dev)
    total = ctypes.c_long(SENT_L)
    rc = L.mxa_ld_window_pairs(p(Xd), snps, indiv, p(lastd), 0.0, 0, p(rowptr), None, None, 0, ctypes.byref(total), 1, p(fd))
    assert (rc, L.mxa_last_error()) == (0, 0), mx.lib.last_error()
    assert total.value == 2_739_845_472 == P["total"] - snps
    col = torch.full((total.value + PAD,), SENT_I, dtype=torch.int32, device=dev)
    val = torch.full((total.value + PAD,), SENTINEL, dtype=torch.float64, device=dev)
    again = ctypes.c_long(SENT_L)
    rc = L.mxa_ld_window_pairs(p(Xd), snps, indiv, p(lastd), 0.0, 0, p(rowptr), p(col), p(val), total.value, ctypes.byref(again), 1, p(fd))
    assert (rc, L.mxa_last_error()) == (0, 0), mx.lib.last_error()
    torch.cuda.synchronize()
    assert again.value == total.value
    assert bool((rowptr[snps + 1:] == SENT_L).all()) and bool((col[total.value:] == SENT_I).all()) and bool((val[total.value:] == SENTINEL).all())
    i = torch.arange(snps, dtype=torch.int64, device=dev)
    assert int(rowptr[0]) == 0 and torch.equal(rowptr[1: snps + 1] - rowptr[:snps], lastd.to(torch.int64) - i)
    # the sampled entries of the rows that are pairs (off the diagonal): position rowptr[i] + d - 1 of the CSR
    si, sj = P["si"], P["sj"]
    off = sj > si
    pos = (P["rowptr"][si] - si) + (sj - si) - 1
    assert (pos[off] > 2 ** 31).sum() * 3 >= off.sum() > 90_000
    posd = torch.from_numpy(pos[off]).to(dev)
    assert np.array_equal(col[posd].cpu().numpy(), sj[off])
    assert np.array_equal(_bits(val[posd].cpu().numpy()), _bits(big["sampled"][off]))
    del val
    torch.cuda.empty_cache()
    for reverse in (False, True):
        prio = -torch.arange(snps, dtype=torch.float64, device=dev) if reverse else None
        want_keep, want_owner, want_kept = lim.full_window_prune_expected(snps, w, reverse, dev)
        assert want_kept == 4
        keep, owner, n_kept, rounds = _prune_csr(mx, snps, rowptr[: snps + 1], col, prio, True)
        what = f"priority {'-i' if reverse else 'NULL'}: "
        assert not (msg := _differ(keep, want_keep)), what + "keep: " + msg
        assert not (msg := _differ(owner, want_owner)), what + "owner: " + msg
        assert n_kept == 4 and 1 <= rounds <= snps, (what, n_kept, rounds)
        print(f"prune on {total.value} pairs, {what}{rounds} rounds")


def test_window_apply_with_rows_past_two_to_the_31(mx, big):
    import torch
    dev = torch.device("cuda", 0)
    P, Xd, fd, lastd = big["P"], big["Xd"], big["fd"], big["lastd"]
    snps, indiv = P["snps"], P["indiv"]
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    n = len(BIG_COLUMNS) + 1
    X = torch.zeros((n, snps), dtype=torch.float64, device=dev)
    for c, k in enumerate(BIG_COLUMNS):
        X[c, k] = 1.0
    X[n - 1] = 1.0
    Y = {}
    for term in (0, 1):
        Yd = torch.full((n + 1, snps), SENTINEL, dtype=torch.float64, device=dev)
        rc = L.mxa_ld_window_apply(p(Xd), snps, indiv, p(lastd), term, p(X), snps, n, p(Yd), snps, 1, p(fd))
        assert (rc, L.mxa_last_error()) == (0, 0), mx.lib.last_error()
        torch.cuda.synchronize()
        assert bool((Yd[n] == SENTINEL).all()), "written outside Y"
        Y[term] = Yd[:n].cpu().numpy()
    assert big["columns"][99_999][3] > 2 ** 31                         # the column's entries lie above flat index 2^31 of the rows
    for c, k in enumerate(BIG_COLUMNS):
        lo, hi, vals, _ = big["columns"][k]
        assert np.array_equal(_bits(Y[0][c, lo: hi + 1]), _bits(vals)), k
        assert np.array_equal(_bits(Y[1][c, lo: hi + 1]), _bits(vals * vals)), k          # term 1: fl(r r)
        for t in (0, 1):
            assert np.all(Y[t][c, :lo] == 0.0) and np.all(Y[t][c, hi + 1:] == 0.0), (t, k)
    S = mx.crossproduct.ld_window_scores(Xd, snps, indiv, lastd, adjust=False, is_plink_format=True, allele_freq=fd).cpu().numpy()
    worst = 0.0
    for i, r in big["windows"].items():
        t = r * r
        bound = 2.0 * len(t) * U * float(t.sum()) * (1.0 - 2.0 ** -40)
        err = abs(Y[1][n - 1, i] - S[i])
        worst = max(worst, err / bound)
        assert err <= bound, (i, err, bound)
    print(f"apply against scores at {snps} SNPs, up to 65 535 terms: worst |err| / bound = {worst:.3e}")
