"""mxa_ld_window_pairs / mxa_ld_window_pairs_pairwise: the pairs i < j <= last[i] with fl(r r) >= min_r2 as CSR, compacted on the device.

  1. the same bits as the filter applied on the host to the output of mxa_ld_window_rows(_pairwise) of the same run -- every shape, window, route, threshold;
  2. from the definition (tests/_ld_ref.py: long double r and the element bound b): with m = 2 |r| b + b^2 + 2 2^-53 r^2 every candidate with r^2 >= t + m is
     present and every one with r^2 < t - m absent; the test asserts FIRST, from the reference alone, that no candidate lies within m of t;
  3. the same bits from both engines, host and device pointers, and with one tile row per group (the running base crosses every group);
  4. the capacity protocol (count-only call, exact capacity, error 25, nothing written at or beyond capacity / total);
  5. mixed host / device output pointers: error 1;   6. the Python wrapper.

Data with LD structure, so that r^2 covers [0, 1]: a SNP is a fresh binomial draw with probability 0.15, else a copy of its predecessor in which each genotype
is redrawn with a per-SNP rate from {0, 0.02, 0.1, 0.3} -- exact duplicates (r = 1) occur."""
import ctypes

import numpy as np
import pytest

import _ld_ref as ref
from _util import pack_plink

pytestmark = pytest.mark.gpu

SENT_L, SENT_I, SENT_D = -7_777_777_777, -777_777, -12345.678
PAD = 67                                   # entries behind every output that must keep the sentinel
SHAPES = [(1, 5), (2, 6), (33, 128), (257, 6), (513, 70), (700, 70), (300, 1030)]
THRESHOLDS = (0.0, 0.2137, 1.0, 2.0)       # check 1; 0.0: every finite off-diagonal window entry (the dense case of the rank arithmetic); 2.0: nothing
DEFINITION_T = (0.0517, 0.2137, 0.7931)    # check 2 (round values such as 0.05 collide exactly with rational r^2 at small indiv)
DEFINITION_SHAPES = [(700, 70), (513, 70), (300, 1030), (257, 6), (33, 128)]
ROUTES = ("", "_pairwise")


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


# ------------------------------------------------------------------------------------------------------------------------------------ data
_CASES = {}


def _genotypes(snps, indiv):
    rng = np.random.default_rng([snps, indiv, 11])
    Z = np.empty((snps, indiv), np.int8)
    for s in range(snps):
        if s == 0 or rng.random() < 0.15:
            Z[s] = rng.binomial(2, rng.uniform(0.05, 0.95), size=indiv)
        else:
            redraw = rng.random(indiv) < (0.0, 0.02, 0.1, 0.3)[int(rng.integers(4))]
            Z[s] = np.where(redraw, rng.integers(0, 3, size=indiv), Z[s - 1])
    const = Z.min(axis=1) == Z.max(axis=1)
    Z[const, 0], Z[const, 1] = 0, 2                                                  # every SNP polymorphic
    return Z, rng


def _case(snps, indiv):
    """X, f: the plain route's data (no missing code, f the data's own frequency); Xp: the same with 10 % missing, where individuals 0, 1, 2 are always
    genotyped and 0, 1 carry 0, 2 -- every pair shares 3 individuals and no SNP is constant on them"""
    key = (snps, indiv)
    if key not in _CASES:
        Z, rng = _genotypes(snps, indiv)
        Zp = Z.copy()
        Zp[:, 0], Zp[:, 1] = 0, 2
        miss = rng.random((snps, indiv)) < 0.10
        miss[:, :3] = False
        _CASES[key] = dict(X=np.ascontiguousarray(pack_plink(Z)), f=Z.astype(np.float64).mean(axis=1) / 2.0, Xp=np.ascontiguousarray(pack_plink(Zp, miss)))
    return _CASES[key]


def _windows(snps):
    """(name, last): the fixed windows at the sub-block edges and the whole matrix, two chromosomes, and at 700 SNPs four seeded geometries"""
    out = [(f"w={w}", ref.fixed_last(snps, w)) for w in sorted({w for w in (0, 1, 31, 32, 33, snps - 1) if w < snps})]
    cut = snps // 2
    if cut >= 1:
        out.append(("two chromosomes", np.where(np.arange(snps) < cut, cut - 1, snps - 1).astype(np.int32)))
    if snps == 700:
        out += [(f"sweep {seed}", ref.sweep_window(snps, seed)) for seed in range(4)]
    return out


# --------------------------------------------------------------------------------------------------------------------------------- calling
def _to(a, device):
    if a is None or not device:
        return a
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _full(n, value, dtype, device):
    if device:
        import torch
        return torch.full((n,), value, dtype={np.int64: torch.int64, np.int32: torch.int32, np.float64: torch.float64}[dtype], device=torch.device("cuda", 0))
    return np.full(n, value, dtype=dtype)


def _host(a, device):
    return a.cpu().numpy() if device else a


def _rows(mx, route, X, snps, indiv, last, f, device=False):
    """mxa_ld_window_rows(_pairwise) at kind 0"""
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    n = int(ref.rowptr_of(last)[-1])
    out = _full(n + PAD, SENT_D, np.float64, device)
    Xa, la, fa = _to(X, device), _to(last, device), _to(f, device)
    rc = getattr(L, "mxa_ld_window_rows" + route)(*([p(Xa), snps, indiv, p(la), p(out), 0] + ([1, p(fa)] if route == "" else [])))
    assert (rc, L.mxa_last_error()) == (0, 0), mx.lib.last_error()
    out = _host(out, device)
    assert np.all(out[n:] == SENT_D)
    return out[:n]


def _pairs(mx, route, X, snps, indiv, last, t, kind, f, capacity, device=False, out_device=None, count_only=False):
    """one call into sentinel-filled outputs with PAD entries behind them; checks that nothing is written where nothing may be; returns
    dict(rc, err, total, rowptr, col, val) with col / val cut to min(total, capacity).  out_device: (rowptr, col, val) on the device, each on its own."""
    import torch
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    od = (device,) * 3 if out_device is None else out_device
    cap = 0 if count_only else int(capacity)
    rowptr, col, val = _full(snps + 1 + PAD, SENT_L, np.int64, od[0]), _full(cap + PAD, SENT_I, np.int32, od[1]), _full(cap + PAD, SENT_D, np.float64, od[2])
    total = ctypes.c_long(SENT_L)
    Xa, la, fa = _to(X, device), _to(last, device), _to(f, device)
    args = [p(Xa), snps, indiv, p(la), float(t), kind, p(rowptr), None if count_only else p(col), None if count_only else p(val), int(capacity), ctypes.byref(total)]
    rc = getattr(L, "mxa_ld_window_pairs" + route)(*(args + ([1, p(fa)] if route == "" else [])))
    err = L.mxa_last_error()
    torch.cuda.synchronize()
    rowptr, col, val = _host(rowptr, od[0]), _host(col, od[1]), _host(val, od[2])
    assert np.all(rowptr[snps + 1:] == SENT_L)
    if err == 1:                                                                     # an argument error: everything untouched
        assert np.all(rowptr == SENT_L) and np.all(col == SENT_I) and np.all(val == SENT_D) and total.value == SENT_L
        return dict(rc=rc, err=err)
    assert err in (0, 25), mx.lib.last_error()
    written = min(total.value, cap) if rc == 0 else cap                              # nothing at or beyond capacity; on success nothing at or beyond total
    assert np.all(col[written:] == SENT_I) and np.all(val[written:] == SENT_D), (route, t, kind, capacity)
    return dict(rc=rc, err=err, total=total.value, rowptr=rowptr[: snps + 1], col=col[:written], val=val[:written])


def _filter(rows, ii, jj, snps, t):
    """the definition applied to the rows entry's kind-0 output: j > i, fl(r r) >= t (false for NaN)"""
    q = rows * rows
    with np.errstate(invalid="ignore"):
        keep = (jj > ii) & (q >= t)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(ii[keep], minlength=snps))]).astype(np.int64)
    return dict(total=int(keep.sum()), rowptr=rowptr, col=jj[keep].astype(np.int32), val=(rows[keep], q[keep]))


def _same(got, want, kind, what):
    assert (got["rc"], got["err"]) == (0, 0) and got["total"] == want["total"], (what, got["rc"], got["err"], got.get("total"), want["total"])
    assert np.array_equal(got["rowptr"], want["rowptr"]), what
    assert np.array_equal(got["col"], want["col"]), what
    assert np.array_equal(got["val"].view(np.int64), want["val"][kind].view(np.int64)), what             # bit for bit


# --------------------------------------------------------------------------------------------------------- 1. same bits as the rows entry
@pytest.mark.parametrize("snps,indiv", SHAPES)
def test_same_bits_as_the_filtered_rows(mx, snps, indiv):
    c = _case(snps, indiv)
    kept = {}
    for name, last in _windows(snps):
        ii, jj = ref.pairs(last)
        for route, X, f in (("", c["X"], c["f"]), ("_pairwise", c["Xp"], None)):
            rows = _rows(mx, route, X, snps, indiv, last, f)
            for t in THRESHOLDS:
                want = _filter(rows, ii, jj, snps, t)
                for kind in (0, 1):
                    _same(_pairs(mx, route, X, snps, indiv, last, t, kind, f, want["total"]), want, kind, (route, name, t, kind))
                if t == 0.0:
                    assert want["total"] == int((np.isfinite(rows) & (jj > ii)).sum())
                if t == 2.0:
                    assert want["total"] == 0 and not want["rowptr"].any()
                kept[route, t] = kept.get((route, t), 0) + want["total"]
    print(f"pairs {snps}x{indiv}: kept over all windows " + ", ".join(f"{r or 'plain'} t={t}: {n}" for (r, t), n in sorted(kept.items())))
    if snps >= 33:
        assert all(kept[r, 2.0] == 0 < kept[r, 1.0] < kept[r, 0.2137] < kept[r, 0.0] for r in ROUTES)     # duplicates (r = 1) occur, and the cutoff cuts


def test_nan_pairs_are_absent(mx):
    """plain: a monomorphic SNP (all 0: sigma = 0, every entry of its row and column is NaN); pairwise: two SNPs without a shared genotyped individual"""
    snps, indiv = 33, 128
    Z, rng = _genotypes(snps, indiv)
    Z[7] = 0
    X, f = np.ascontiguousarray(pack_plink(Z)), Z.astype(np.float64).mean(axis=1) / 2.0
    Zp, miss = Z.copy(), rng.random((snps, indiv)) < 0.10
    Zp[7] = Z[6]
    miss[11], miss[20] = np.arange(indiv) % 2 == 0, np.arange(indiv) % 2 == 1
    Xp = np.ascontiguousarray(pack_plink(Zp, miss))
    last = ref.fixed_last(snps, snps - 1)
    ii, jj = ref.pairs(last)
    for route, Xr, fr, nan_pair in (("", X, f, (7, 12)), ("_pairwise", Xp, None, (11, 20))):
        rows = _rows(mx, route, Xr, snps, indiv, last, fr)
        k = np.flatnonzero((ii == nan_pair[0]) & (jj == nan_pair[1]))[0]
        assert np.isnan(rows[k]), route
        if route == "":
            assert np.isnan(rows[(ii != jj) & ((ii == 7) | (jj == 7))]).all()
        for t in (0.0, 0.2137):
            want = _filter(rows, ii, jj, snps, t)
            got = _pairs(mx, route, Xr, snps, indiv, last, t, 0, fr, want["total"])
            _same(got, want, 0, (route, t))
            i, j = nan_pair
            assert j not in got["col"][got["rowptr"][i]: got["rowptr"][i + 1]] and np.isfinite(got["val"]).all() and 0 < got["total"] < len(ii) - snps


# -------------------------------------------------------------------------------------------------------------- 2. from the definition
@pytest.mark.parametrize("route", ROUTES, ids=["plain", "pairwise"])
@pytest.mark.parametrize("snps,indiv", DEFINITION_SHAPES)
def test_from_the_definition(mx, snps, indiv, route):
    c = _case(snps, indiv)
    if route == "":
        X, f = c["X"], c["f"]
        pc = ref.plain_case(X, indiv, f)
        r, b = pc["r"], pc["b"]
        assert np.all(pc["sigma2"] > 0)
    else:
        X, f = c["Xp"], None
        r = ref.pairwise_restate(X, indiv)["r"]
        b = ref.pairwise_bound(r)
    last = ref.fixed_last(snps, snps - 1)                                            # every pair i < j is a candidate
    iu, ju = np.triu_indices(snps, k=1)
    r, b = r[iu, ju], b[iu, ju]
    assert np.isfinite(r.astype(np.float64)).all() and np.isfinite(b).all()
    r2 = r * r                                                                        # long double
    m = (2 * np.abs(r) * b + b.astype(ref.LD) * b + 2 * ref.LD(ref.U) * r2)
    for t in DEFINITION_T:
        # the condition, from the reference alone: no candidate within m of t, so nothing is left undecided
        must, must_not = r2 >= t + m, r2 < t - m
        assert np.all(must | must_not), (t, int((~(must | must_not)).sum()))
        assert must.sum() >= 15, (t, int(must.sum()))
        want_rowptr = np.concatenate([[0], np.cumsum(np.bincount(iu[must], minlength=snps))])
        got = _pairs(mx, route, X, snps, indiv, last, t, 0, f, int(must.sum()) + 3)
        q = ref.worst_ratio(got["val"], r[must], b[must]) if got["rc"] == 0 and got["total"] == must.sum() else float("inf")
        gap = float(np.min(np.abs(r2 - t) / np.where(m > 0, m, ref.LD(ref.U) ** 2)))                  # m = 0 only where r = 0 and b = 0
        print(f"definition {snps}x{indiv} {route or 'plain'} t={t}: {int(must.sum())} pairs, smallest |r^2 - t| / m {gap:.3g}, worst |err| / bound {q:.3f}")
        assert (got["rc"], got["err"], got["total"]) == (0, 0, int(must.sum()))
        assert np.array_equal(got["rowptr"], want_rowptr) and np.array_equal(got["col"], ju[must])
        assert q <= 1.0, q


# -------------------------------------------------------------------------------------------------------------- 3. same bits everywhere
CONFIGS = [("i8", False, None), ("f4", True, None), ("i8", True, "1"), ("f4", False, "1")]     # (engine, device pointers, MXA_LD_PAIRWISE_SCRATCH_MB)


@pytest.mark.parametrize("snps,indiv", SHAPES)
def test_same_bits_from_every_engine_pointer_kind_and_scratch_size(mx, monkeypatch, snps, indiv):
    c = _case(snps, indiv)
    for name, last in _windows(snps):
        for route, X, f in (("", c["X"], c["f"]), ("_pairwise", c["Xp"], None)):
            for t, kind in ((0.0, 1), (0.2137, 0)):
                monkeypatch.delenv("MXA_XPROD_ENGINE", raising=False)
                monkeypatch.delenv("MXA_LD_PAIRWISE_SCRATCH_MB", raising=False)
                cnt = _pairs(mx, route, X, snps, indiv, last, t, kind, f, 0, count_only=True)
                first = _pairs(mx, route, X, snps, indiv, last, t, kind, f, cnt["total"])
                assert (first["rc"], first["err"], first["total"]) == (0, 0, cnt["total"]) and np.array_equal(first["rowptr"], cnt["rowptr"])
                for engine, device, scratch in CONFIGS:
                    monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
                    if scratch:
                        monkeypatch.setenv("MXA_LD_PAIRWISE_SCRATCH_MB", scratch)
                    else:
                        monkeypatch.delenv("MXA_LD_PAIRWISE_SCRATCH_MB", raising=False)
                    got = _pairs(mx, route, X, snps, indiv, last, t, kind, f, cnt["total"], device=device)
                    what = (route, name, t, engine, device, scratch)
                    assert (got["rc"], got["err"], got["total"]) == (0, 0, cnt["total"]), what
                    assert np.array_equal(got["rowptr"], first["rowptr"]) and np.array_equal(got["col"], first["col"]), what
                    assert np.array_equal(got["val"].view(np.int64), first["val"].view(np.int64)), what


# ------------------------------------------------------------------------------------------------------------------ 4. capacity protocol
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("route", ROUTES, ids=["plain", "pairwise"])
def test_capacity_protocol(mx, route, device):
    snps, indiv, t = 513, 70, 0.2137
    c = _case(snps, indiv)
    X, f = (c["X"], c["f"]) if route == "" else (c["Xp"], None)
    last = ref.fixed_last(snps, 300)
    ii, jj = ref.pairs(last)
    want = _filter(_rows(mx, route, X, snps, indiv, last, f, device), ii, jj, snps, t)
    total = want["total"]
    assert total > 1000 and 0 < want["rowptr"][256] < want["rowptr"][512] == total                # pairs in both tile rows that can hold one (SNP 512 is the last)
    cnt = _pairs(mx, route, X, snps, indiv, last, t, 0, f, -5, device=device, count_only=True)       # capacity is ignored
    assert (cnt["rc"], cnt["err"], cnt["total"]) == (0, 0, total) and np.array_equal(cnt["rowptr"], want["rowptr"])
    for kind in (0, 1):
        _same(_pairs(mx, route, X, snps, indiv, last, t, kind, f, total, device=device), want, kind, ("exact", kind))
        _same(_pairs(mx, route, X, snps, indiv, last, t, kind, f, total + 5, device=device), want, kind, ("roomy", kind))
    for capacity in (total - 1, 0):
        got = _pairs(mx, route, X, snps, indiv, last, t, 0, f, capacity, device=device)
        assert (got["rc"], got["err"], got["total"]) == (1, 25, total), capacity
        assert np.array_equal(got["rowptr"], want["rowptr"])
    _pairs(mx, route, X, snps, indiv, last, t, 0, f, 0, device=device)
    code, msg = mx.lib.last_error()
    assert code == 25 and str(total) in msg and " 0" in msg, msg                                    # the message names both numbers
    bad = _pairs(mx, route, X, snps, indiv, last, t, 0, f, -1, device=device)                        # capacity < 0 on a filling call
    assert (bad["rc"], bad["err"]) == (1, 1)


# ------------------------------------------------------------------------------------------------------------------ 5. mixed pointers
@pytest.mark.parametrize("route", ROUTES, ids=["plain", "pairwise"])
def test_mixed_host_and_device_outputs_are_rejected(mx, route):
    snps, indiv = 33, 128
    c = _case(snps, indiv)
    X, f = (c["X"], c["f"]) if route == "" else (c["Xp"], None)
    last = ref.fixed_last(snps, 5)
    for od in [(True, False, False), (False, True, True), (False, True, False), (True, True, False), (True, False, True)]:
        got = _pairs(mx, route, X, snps, indiv, last, 0.2137, 0, f, 100, out_device=od)
        assert (got["rc"], got["err"]) == (1, 1), od
    got = _pairs(mx, route, X, snps, indiv, last, 0.2137, 0, f, 100, device=False, out_device=(True, True, True))   # host inputs, device outputs: legal
    assert (got["rc"], got["err"]) == (0, 0)


# ----------------------------------------------------------------------------------------------------------------------------- 6. Python
@pytest.mark.parametrize("pairwise", [False, True], ids=["plain", "pairwise"])
def test_python_wrapper(mx, pairwise):
    import torch
    snps, indiv, w, t = 513, 70, 33, 0.2137
    c = _case(snps, indiv)
    X, f = (c["Xp"], None) if pairwise else (c["X"], c["f"])
    last = ref.fixed_last(snps, w)
    ii, jj = ref.pairs(last)
    want = _filter(_rows(mx, "_pairwise" if pairwise else "", X, snps, indiv, last, f), ii, jj, snps, t)
    kw = dict(min_r2=t, pairwise=pairwise, is_plink_format=True, allele_freq=f)
    dev = torch.device("cuda", 0)
    for kind, k in (("r", 0), ("r2", 1)):
        for device in (False, True):
            Xa = torch.from_numpy(X).to(dev) if device else X
            fa = torch.from_numpy(f).to(dev) if device and f is not None else f
            la = torch.from_numpy(last).to(dev) if device else last
            for args in (dict(window=w), dict(last=la), dict(window=w, capacity=want["total"] + 9), dict(last=la, capacity=want["total"])):
                rowptr, col, val = mx.crossproduct.ld_pairs(Xa, snps, indiv, kind=kind, **dict(kw, allele_freq=fa), **args)
                if device:
                    assert rowptr.device.type == col.device.type == val.device.type == "cuda"
                    rowptr, col, val = rowptr.cpu().numpy(), col.cpu().numpy(), val.cpu().numpy()
                assert rowptr.dtype == np.int64 and col.dtype == np.int32 and val.dtype == np.float64
                assert np.array_equal(rowptr, want["rowptr"]) and np.array_equal(col, want["col"]) and np.array_equal(val.view(np.int64), want["val"][k].view(np.int64))
    with pytest.raises(RuntimeError, match=str(want["total"])):
        mx.crossproduct.ld_pairs(X, snps, indiv, window=w, capacity=want["total"] - 1, **kw)
