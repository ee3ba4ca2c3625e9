"""mxa_ld_prune_csr / mxa_ld_window_prune / mxa_ld_window_prune_pairwise: the greedy selection on the pairs graph (LD pruning and clumping), on the device.

  1. the graph step on hand-made CSRs, host and device pointers, against the sequential walk (tests/_ld_prune_ref.py): keep, owner, n_kept exactly, `rounds`
     equal between the pointer kinds, sentinels behind keep / owner intact;
  2. the window entries against the walk on the CSR mxa_ld_window_pairs(_pairwise) returns in the same run: every shape, window, route, threshold, priority;
  3. from the definition (tests/_ld_ref.py, nothing of the library): the edge set r^2 >= t + m of the long-double reference, after asserting that no candidate
     lies within m of t; plus independence and maximality checked directly;
  4. the same result from both engines, host / device pointers and one tile row per scratch group;
  5. the argument errors, outputs untouched;   6. the Python wrappers.

Data, shapes, windows and routes: those of tests/test_ld_pairs_gpu.py, same seeds."""
import ctypes

import numpy as np
import pytest

import _ld_ref as ref
from _ld_prune_ref import csr_of_edges, neighbours, ref_greedy
from _util import pack_plink

pytestmark = pytest.mark.gpu

SENT_L, SENT_I, SENT_B, SENT_R = -7_777_777_777, -777_777, 0xAB, -777
PAD = 67                                   # entries behind every output that must keep the sentinel
SHAPES = [(1, 5), (2, 6), (33, 128), (257, 6), (513, 70), (700, 70), (300, 1030)]
THRESHOLDS = (0.0, 0.2137, 1.0, 2.0)
DEFINITION_T = (0.0517, 0.2137, 0.7931)
DEFINITION_SHAPES = [(700, 70), (513, 70), (300, 1030)]
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
    genotyped and 0, 1 carry 0, 2; prio: the three priorities of the checks (None, -MAF of the data, seeded random with deliberate ties)"""
    key = (snps, indiv)
    if key not in _CASES:
        Z, rng = _genotypes(snps, indiv)
        Zp = Z.copy()
        Zp[:, 0], Zp[:, 1] = 0, 2
        miss = rng.random((snps, indiv)) < 0.10
        miss[:, :3] = False
        f = Z.astype(np.float64).mean(axis=1) / 2.0
        ties = np.random.default_rng([snps, indiv, 12]).integers(0, 8, size=snps).astype(np.float64)
        _CASES[key] = dict(X=np.ascontiguousarray(pack_plink(Z)), f=f, Xp=np.ascontiguousarray(pack_plink(Zp, miss)),
                           prio=(("NULL", None), ("-MAF", -np.minimum(f, 1.0 - f)), ("ties", ties)))
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
_TORCH = {np.int64: "int64", np.int32: "int32", np.float64: "float64", np.uint8: "uint8"}


def _to(a, device):
    if a is None or not device:
        return a
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _full(n, value, dtype, device):
    if device:
        import torch
        return torch.full((n,), value, dtype=getattr(torch, _TORCH[dtype]), device=torch.device("cuda", 0))
    return np.full(n, value, dtype=dtype)


def _host(a, device):
    return a.cpu().numpy() if device else a


def _outputs(snps, out_device, owner):
    """sentinel-filled keep / owner (PAD entries behind them), n_kept, rounds.  out_device: (keep, owner) on the device, each on its own"""
    keep = _full(snps + PAD, SENT_B, np.uint8, out_device[0])
    own = _full(snps + PAD, SENT_I, np.int32, out_device[1]) if owner else None
    return keep, own, ctypes.c_long(SENT_L), ctypes.c_int(SENT_R)


def _collect(mx, rc, snps, keep, own, n_kept, rounds, out_device, what):
    """the result of one call; checks the sentinels behind the outputs, and on an argument error everywhere"""
    import torch
    L = mx.lib.check_library_handle()
    err = L.mxa_last_error()
    torch.cuda.synchronize()
    keep = _host(keep, out_device[0])
    own = None if own is None else _host(own, out_device[1])
    assert np.all(keep[snps:] == SENT_B) and (own is None or np.all(own[snps:] == SENT_I)), what
    if rc != 0:
        assert np.all(keep == SENT_B) and (own is None or np.all(own == SENT_I)) and n_kept.value == SENT_L and rounds.value == SENT_R, what
        return dict(rc=rc, err=err)
    assert err == 0 and set(np.unique(keep[:snps])) <= {0, 1}, (what, mx.lib.last_error())
    return dict(rc=rc, err=err, keep=keep[:snps].astype(bool), owner=None if own is None else own[:snps].copy(), n_kept=n_kept.value, rounds=rounds.value)


def _prune_csr(mx, snps, rowptr, col, prio, device=False, owner=True, in_device=None, out_device=None, keep_null=False):
    """mxa_ld_prune_csr.  in_device: (rowptr, col, priority) on the device, each on its own; default: all as `device`"""
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    ind = (device,) * 3 if in_device is None else in_device
    od = (device,) * 2 if out_device is None else out_device
    keep, own, n_kept, rounds = _outputs(snps, od, owner)
    ra, ca, pa = _to(rowptr, ind[0]), _to(col, ind[1]), _to(prio, ind[2])
    rc = L.mxa_ld_prune_csr(snps, p(ra), p(ca) if len(col) else None, p(pa), None if keep_null else p(keep), p(own), ctypes.byref(n_kept), ctypes.byref(rounds))
    return _collect(mx, rc, snps, keep, own, n_kept, rounds, od, ("csr", snps, device, in_device, out_device))


def _prune_window(mx, route, X, snps, indiv, last, t, prio, f, device=False, owner=True, out_device=None, keep_null=False):
    """mxa_ld_window_prune(_pairwise)"""
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    od = (device,) * 2 if out_device is None else out_device
    keep, own, n_kept, rounds = _outputs(snps, od, owner)
    Xa, la, fa, pa = _to(X, device), _to(last, device), _to(f, device), _to(prio, device)
    args = [p(Xa), snps, indiv, p(la), float(t), p(pa), None if keep_null else p(keep), p(own), ctypes.byref(n_kept), ctypes.byref(rounds)]
    rc = getattr(L, "mxa_ld_window_prune" + route)(*(args + ([1, p(fa)] if route == "" else [])))
    return _collect(mx, rc, snps, keep, own, n_kept, rounds, od, ("window", route, snps, t, device, out_device))


def _pairs(mx, route, X, snps, indiv, last, t, f):
    """(rowptr, col) of mxa_ld_window_pairs(_pairwise): the count-only call, then the exactly sized filling call"""
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    rowptr, total = np.zeros(snps + 1, np.int64), ctypes.c_long(0)
    tail = [1, p(f)] if route == "" else []
    fn = getattr(L, "mxa_ld_window_pairs" + route)
    assert fn(p(X), snps, indiv, p(last), float(t), 1, p(rowptr), None, None, 0, ctypes.byref(total), *tail) == 0, mx.lib.last_error()
    col, val = np.zeros(total.value, np.int32), np.zeros(total.value, np.float64)
    assert fn(p(X), snps, indiv, p(last), float(t), 1, p(rowptr), p(col), p(val), total.value, ctypes.byref(total), *tail) == 0, mx.lib.last_error()
    return rowptr, col


def _same_as_walk(got, snps, rowptr, col, prio, what):
    keep, owner = ref_greedy(snps, rowptr, col, prio)
    assert (got["rc"], got["err"]) == (0, 0), what
    assert np.array_equal(got["keep"], keep), what
    assert got["n_kept"] == int(keep.sum()), what
    assert 1 <= got["rounds"] <= snps, (what, got["rounds"])
    if got["owner"] is not None:
        assert np.array_equal(got["owner"], owner), what
    return keep, owner


# ------------------------------------------------------------------------------------------------- 1. the graph step on hand-made graphs
def _path(n):
    return [(i, i + 1) for i in range(n - 1)]


def _clique(vs):
    return [(a, b) for k, a in enumerate(vs) for b in vs[k + 1:]]


def _banded(n, bandwidth, seed):
    rng = np.random.default_rng([n, bandwidth, seed])
    i = rng.integers(0, n - 1, size=6 * n)
    j = np.minimum(i + rng.integers(1, bandwidth + 1, size=6 * n), n - 1)
    return [(int(a), int(b)) for a, b in zip(i, j) if a < b]


def _rand(n, seed):
    return np.random.default_rng([n, seed]).random(n)


_INF = np.array([np.inf, -np.inf, 0.0, -0.0, 1.5, -np.inf, np.inf, 0.0, 2.0, -1.0, np.inf, -0.0])
GRAPHS = [("1 SNP", 1, [], [None, np.array([3.0])]),
          ("2 SNPs, edge", 2, [(0, 1)], [None, np.array([2.0, 1.0]), np.array([1.0, 1.0])]),
          ("2 SNPs, no edge", 2, [], [None, np.array([2.0, 1.0])]),
          ("empty on 300", 300, [], [None, _rand(300, 1)]),
          ("path 700", 700, _path(700), [None, -np.arange(700.0), _rand(700, 2)]),
          ("star, hub first", 300, [(0, v) for v in range(1, 300)], [None, _rand(300, 3)]),
          ("star, hub last", 300, [(v, 299) for v in range(299)], [None, -np.arange(300.0), _rand(300, 4)]),
          ("clique of 40", 40, _clique(list(range(40))), [None, _rand(40, 5), -np.arange(40.0)]),
          ("two cliques and a bridge", 70, _clique(list(range(30))) + _clique(list(range(30, 70))) + [(29, 30)], [None, _rand(70, 6), -np.arange(70.0)]),
          ("all priorities equal", 200, _banded(200, 9, 7), [np.full(200, 0.25)]),
          ("priorities with +-inf", 12, _banded(12, 4, 8) + _path(12), [_INF, -_INF]),
          ("banded on 1000", 1000, _banded(1000, 64, 9), [_rand(1000, s) for s in (10, 11, 12, 13)] + [None])]


@pytest.mark.parametrize("name,snps,edges,priorities", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_graph_step_on_hand_made_graphs(mx, name, snps, edges, priorities):
    rowptr, col = csr_of_edges(snps, edges)
    for k, prio in enumerate(priorities):
        got = {device: _prune_csr(mx, snps, rowptr, col, prio, device=device) for device in (False, True)}
        for device in (False, True):
            keep, owner = _same_as_walk(got[device], snps, rowptr, col, prio, (name, k, device))
        assert got[False]["rounds"] == got[True]["rounds"], (name, k)
        print(f"{name}, priority {k}: kept {int(keep.sum())} of {snps}, rounds {got[True]['rounds']}")
        if name == "path 700" and prio is None:
            assert np.array_equal(keep, np.arange(700) % 2 == 0) and got[True]["rounds"] >= 350
        if name == "star, hub first" and prio is None:
            assert keep[0] and keep.sum() == 1 and np.all(owner == 0)
        if name == "star, hub last" and prio is None:
            assert not keep[299] and keep.sum() == 299 and owner[299] == 0
        if name == "clique of 40":
            assert keep.sum() == 1
        if not edges:
            assert keep.all() and got[True]["rounds"] <= 1
    # the inputs on the device each on its own, outputs on the host and the other way round
    prio = priorities[-1]
    first = _prune_csr(mx, snps, rowptr, col, prio)
    for ind in [(True, False, False), (False, True, False), (False, False, True), (True, True, False)]:
        for od in (False, True):
            other = _prune_csr(mx, snps, rowptr, col, prio, in_device=ind, out_device=(od, od))
            assert all(np.array_equal(other[k], first[k]) for k in ("keep", "owner", "n_kept", "rounds")), (name, ind, od)


# ------------------------------------------------------------------------------- 2. the window entries against the pairs entry of the run
@pytest.mark.parametrize("route", ROUTES, ids=["plain", "pairwise"])
@pytest.mark.parametrize("snps,indiv", SHAPES)
def test_window_entries_against_the_walk_on_the_pairs_entry(mx, snps, indiv, route):
    c = _case(snps, indiv)
    X, f = (c["X"], c["f"]) if route == "" else (c["Xp"], None)
    kept = {}
    for name, last in _windows(snps):
        for t in THRESHOLDS:
            rowptr, col = _pairs(mx, route, X, snps, indiv, last, t, f)
            for pname, prio in c["prio"]:
                got = _prune_window(mx, route, X, snps, indiv, last, t, prio, f)
                keep, _ = _same_as_walk(got, snps, rowptr, col, prio, (route, name, t, pname))
                kept[t, pname] = kept.get((t, pname), 0) + int(keep.sum())
                if t == 2.0:
                    assert len(col) == 0 and keep.all() and got["rounds"] <= 1
    print(f"prune {snps}x{indiv} {route or 'plain'}: kept over all windows " + ", ".join(f"t={t} {p}: {n}" for (t, p), n in sorted(kept.items())))
    if snps >= 33:                                                                   # duplicates (r = 1) occur: an edge at every t <= 1 drops a SNP
        assert all(max(kept[t, p] for t in (0.0, 0.2137, 1.0)) < kept[2.0, p] for p in ("NULL", "-MAF", "ties"))


# -------------------------------------------------------------------------------------------------------------- 3. from the definition
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
    m = (2 * np.abs(r) * b + b.astype(ref.LD) * b + 2 * ref.LD(ref.U) * r2)           # the margin of the pairs test
    for t in DEFINITION_T:
        # the condition, from the reference alone: no candidate within m of t, so the edge set is decided
        must, must_not = r2 >= t + m, r2 < t - m
        assert np.all(must | must_not), (t, int((~(must | must_not)).sum()))
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(iu[must], minlength=snps))]).astype(np.int64)
        col = ju[must].astype(np.int32)
        adj = np.zeros((snps, snps), dtype=bool)
        adj[iu[must], ju[must]] = adj[ju[must], iu[must]] = True
        for pname, prio in c["prio"]:
            got = _prune_window(mx, route, X, snps, indiv, last, t, prio, f)
            keep, owner = _same_as_walk(got, snps, rowptr, col, prio, (route, t, pname))
            k = got["keep"]
            assert not adj[np.ix_(k, k)].any(), (route, t, pname)                     # independent: no kept pair has r^2 >= t + m
            assert adj[np.ix_(~k, k)].any(axis=1).all(), (route, t, pname)            # maximal: every dropped SNP has a kept neighbour
            assert adj[np.flatnonzero(~k), got["owner"][~k]].all() and k[got["owner"]].all(), (route, t, pname)
            print(f"definition {snps}x{indiv} {route or 'plain'} t={t} {pname}: {int(must.sum())} edges, kept {int(k.sum())}, rounds {got['rounds']}")


# -------------------------------------------------------------------------------------------------------------- 4. same result everywhere
CONFIGS = [("i8", False, None), ("f4", True, None), ("i8", True, "1"), ("f4", False, "1")]     # (engine, device pointers, MXA_LD_PAIRWISE_SCRATCH_MB)


@pytest.mark.parametrize("snps,indiv", [(513, 70), (700, 70)])
def test_same_result_from_every_engine_pointer_kind_and_scratch_size(mx, monkeypatch, snps, indiv):
    c = _case(snps, indiv)
    for name, last in _windows(snps):
        for route, X, f in (("", c["X"], c["f"]), ("_pairwise", c["Xp"], None)):
            for (pname, prio), t in zip(c["prio"], (0.0, 0.2137, 0.2137)):
                monkeypatch.delenv("MXA_XPROD_ENGINE", raising=False)
                monkeypatch.delenv("MXA_LD_PAIRWISE_SCRATCH_MB", raising=False)
                first = _prune_window(mx, route, X, snps, indiv, last, t, prio, f)
                assert (first["rc"], first["err"]) == (0, 0)
                for engine, device, scratch in CONFIGS:
                    monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
                    if scratch:
                        monkeypatch.setenv("MXA_LD_PAIRWISE_SCRATCH_MB", scratch)
                    else:
                        monkeypatch.delenv("MXA_LD_PAIRWISE_SCRATCH_MB", raising=False)
                    got = _prune_window(mx, route, X, snps, indiv, last, t, prio, f, device=device)
                    what = (route, name, t, pname, engine, device, scratch)
                    assert (got["rc"], got["err"]) == (0, 0), what
                    assert all(np.array_equal(got[k], first[k]) for k in ("keep", "owner", "n_kept", "rounds")), what


# ------------------------------------------------------------------------------------------------------------------------------ 5. errors
def test_errors_of_the_window_entries(mx):
    snps, indiv = 33, 128
    c = _case(snps, indiv)
    last = ref.fixed_last(snps, 5)
    nan = c["prio"][1][1].copy()
    nan[17] = np.nan
    inf = c["prio"][1][1].copy()
    inf[3], inf[20] = np.inf, -np.inf
    for route, X, f in (("", c["X"], c["f"]), ("_pairwise", c["Xp"], None)):
        good = _prune_window(mx, route, X, snps, indiv, last, 0.2137, c["prio"][1][1], f)
        assert (good["rc"], good["err"]) == (0, 0)
        for device in (False, True):
            bad = _prune_window(mx, route, X, snps, indiv, last, 0.2137, nan, f, device=device)
            assert (bad["rc"], bad["err"]) == (1, 1), (route, device, "NaN priority")
            assert "NaN" in mx.lib.last_error()[1]
            ok = _prune_window(mx, route, X, snps, indiv, last, 0.2137, inf, f, device=device)                 # +-inf is legal
            assert (ok["rc"], ok["err"]) == (0, 0) and ok["keep"][20]
        for od in [(True, False), (False, True)]:
            bad = _prune_window(mx, route, X, snps, indiv, last, 0.2137, None, f, out_device=od)
            assert (bad["rc"], bad["err"]) == (1, 1), (route, od)
        bad = _prune_window(mx, route, X, snps, indiv, last, 0.2137, None, f, keep_null=True)
        assert (bad["rc"], bad["err"]) == (1, 1), (route, "keep NULL")
        for what, kw in (("min_r2 negative", dict(t=-0.5)), ("min_r2 NaN", dict(t=float("nan"))), ("last decreasing", dict(last=last[::-1].copy()))):
            args = dict(dict(last=last, t=0.2137), **kw)
            bad = _prune_window(mx, route, X, snps, indiv, args["last"], args["t"], None, f)                   # what the pairs entry rejects
            assert (bad["rc"], bad["err"]) == (1, 1), (route, what)
        for device in (False, True):                                                                            # owner == NULL: its pass is skipped
            lone = _prune_window(mx, route, X, snps, indiv, last, 0.2137, c["prio"][1][1], f, device=device, owner=False)
            assert (lone["rc"], lone["err"]) == (0, 0) and lone["owner"] is None
            assert np.array_equal(lone["keep"], good["keep"]) and (lone["n_kept"], lone["rounds"]) == (good["n_kept"], good["rounds"])
        host_in_device_out = _prune_window(mx, route, X, snps, indiv, last, 0.2137, c["prio"][1][1], f, device=False, out_device=(True, True))   # legal
        assert np.array_equal(host_in_device_out["keep"], good["keep"]) and np.array_equal(host_in_device_out["owner"], good["owner"])
    bad = _prune_window(mx, "", c["X"], snps, indiv, last, 0.2137, None, None)                                  # the plain route needs the frequencies
    assert (bad["rc"], bad["err"]) == (1, 1)


BAD_CSR = [("descending column", [0, 2, 3, 3, 3], [3, 1, 2]), ("repeated column", [0, 2, 3, 3, 3], [2, 2, 3]), ("column equal to its row", [0, 1, 2, 2, 2], [1, 1]),
           ("column below its row", [0, 1, 2, 3, 3], [1, 2, 0]), ("column equal to snps", [0, 1, 2, 2, 2], [1, 4]), ("column negative", [0, 1, 1, 1, 1], [-1]),
           ("decreasing rowptr", [0, 2, 1, 3, 3], [1, 2, 3]), ("rowptr[0] not 0", [1, 2, 3, 3, 3], [1, 2, 3])]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("what,rowptr,col", BAD_CSR, ids=[b[0] for b in BAD_CSR])
def test_errors_of_the_graph_step(mx, what, rowptr, col, device):
    snps = 4
    rowptr, col = np.array(rowptr, np.int64), np.array(col, np.int32)
    bad = _prune_csr(mx, snps, rowptr, col, None, device=device)
    assert (bad["rc"], bad["err"]) == (1, 1), what
    if what == "descending column":                                                                              # once: the errors that are not the CSR's
        rowptr, col = csr_of_edges(snps, [(0, 1), (1, 2), (2, 3)])
        good = _prune_csr(mx, snps, rowptr, col, None, device=device)
        assert (good["rc"], good["err"]) == (0, 0) and np.array_equal(good["keep"], [True, False, True, False]) and np.array_equal(good["owner"], [0, 0, 2, 2])
        for w, kw in (("NaN priority", dict(prio=np.array([0.5, np.nan, 1.0, 2.0]))), ("keep NULL", dict(prio=None, keep_null=True)),
                      ("mixed outputs", dict(prio=None, out_device=(True, False))), ("mixed outputs", dict(prio=None, out_device=(False, True)))):
            bad = _prune_csr(mx, snps, rowptr, col, device=device, **kw)
            assert (bad["rc"], bad["err"]) == (1, 1), w
        lone = _prune_csr(mx, snps, rowptr, col, None, device=device, owner=False)
        assert (lone["rc"], lone["err"]) == (0, 0) and np.array_equal(lone["keep"], good["keep"]) and lone["rounds"] == good["rounds"]


# ----------------------------------------------------------------------------------------------------------------------------- 6. Python
@pytest.mark.parametrize("pairwise", [False, True], ids=["plain", "pairwise"])
def test_python_wrappers(mx, pairwise):
    import torch
    snps, indiv, w, t = 513, 70, 33, 0.2137
    c = _case(snps, indiv)
    X, f = (c["Xp"], None) if pairwise else (c["X"], c["f"])
    last = ref.fixed_last(snps, w)
    rowptr, col = _pairs(mx, "_pairwise" if pairwise else "", X, snps, indiv, last, t, f)
    dev = torch.device("cuda", 0)
    for pname, prio in c["prio"]:
        keep, owner = ref_greedy(snps, rowptr, col, prio)
        for device in (False, True):
            Xa = torch.from_numpy(X).to(dev) if device else X
            fa = torch.from_numpy(f).to(dev) if device and f is not None else f
            la = torch.from_numpy(last).to(dev) if device else last
            pa = torch.from_numpy(prio).to(dev) if device and prio is not None else prio
            kw = dict(min_r2=t, priority=pa, pairwise=pairwise, is_plink_format=True, allele_freq=fa)
            for args in (dict(window=w), dict(last=la)):
                k = mx.crossproduct.ld_prune(Xa, snps, indiv, **kw, **args)
                k2, o2 = mx.ld_prune(Xa, snps, indiv, return_owner=True, **kw, **args)
                k3, o3, rounds = mx.crossproduct.ld_prune(Xa, snps, indiv, return_owner=True, return_rounds=True, **kw, **args)
                if device:
                    assert k.device.type == k2.device.type == o2.device.type == "cuda" and k.dtype == torch.bool and o2.dtype == torch.int32
                    k, k2, o2, k3, o3 = (x.cpu().numpy() for x in (k, k2, o2, k3, o3))
                assert k.dtype == np.bool_ and o2.dtype == np.int32 and 1 <= rounds <= snps
                assert np.array_equal(k, keep) and np.array_equal(k2, keep) and np.array_equal(o2, owner) and np.array_equal(k3, keep) and np.array_equal(o3, owner)
            ra, ca = (torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev)) if device else (rowptr, col)
            k = mx.ld_prune_csr(ra, ca, priority=pa)
            k2, o2 = mx.crossproduct.ld_prune_csr(ra, ca, priority=pa, return_owner=True)
            if device:
                assert k.device.type == o2.device.type == "cuda"
                k, k2, o2 = k.cpu().numpy(), k2.cpu().numpy(), o2.cpu().numpy()
            assert np.array_equal(k, keep) and np.array_equal(k2, keep) and np.array_equal(o2, owner), pname
    start, nb = neighbours(snps, rowptr, col)
    assert int(start[-1]) == 2 * len(col) > 0 and len(nb) == 2 * len(col)
    with pytest.raises(RuntimeError, match="ascending"):
        mx.ld_prune_csr(np.array([0, 2, 2, 2], np.int64), np.array([2, 1], np.int32))
