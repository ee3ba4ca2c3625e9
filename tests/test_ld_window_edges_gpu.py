"""The eight windowed LD entries against references from the definition (tests/_ld_ref.py: exact integer crossproducts, the LD map in long double, an
element-wise bound derived from the library's three float64 lines -- mxa_ld is part of no reference here), at the edges the other LD tests never ran at:

  a. small and ragged shapes: indiv % 4 = 0 .. 3, indiv below / at / one past one 128-genotype LDS stage, snps = 1 and below / at / one past a 32-row sub-block
     and a 256-row tile; every entry, both engines, host and device pointers, fixed windows and a two-chromosome `last`;
  b. 32 seeded window geometries at 700 x 70 (tests/test_ld_window_sweep_cpu.py asserts what they hold);
  c. the FP4 -> int8 engine rule at its limits on the windowed routes, with the fp32 accumulator at the top of its 24 bits;
  d. more than 2^31 stored entries: rowptr[] and gi * ldb as 64-bit indices.

Every test prints its worst |err| / bound (run with -s)."""
import numpy as np
import pytest

import _ld_ref as ref
from _util import pack_plink

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
PAD = 67                                   # doubles behind the result that must keep the sentinel
EDGE_SHAPES = [(1, 5), (2, 6), (31, 3), (32, 127), (33, 128), (64, 129), (255, 130), (256, 254), (257, 6), (513, 70), (300, 1030)]
PLAIN = ("mxa_ld_band", "mxa_ld_scores", "mxa_ld_window_rows", "mxa_ld_window_scores")


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


# ------------------------------------------------------------------------------------------------------------------------------ calling
def _call(mx, entry, X, snps, indiv, win, nout, flag, f=None, device=False, ldb=None, is_plink=1):
    """a C entry (win: the window of the fixed entries, `last` of the general ones) into nout + PAD doubles pre-filled with a sentinel; asserts success and
    that nothing is written beyond nout; returns the nout doubles as numpy"""
    L = mx.lib.check_library_handle()
    p = mx.lib.ptr
    if device:
        import torch
        dev = torch.device("cuda", 0)
        to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        out = torch.full((nout + PAD,), SENTINEL, dtype=torch.float64, device=dev)
    else:
        to = lambda a: a
        out = np.full(nout + PAD, SENTINEL, dtype=np.float64)
    Xa, fa = to(X), to(f)
    w = int(win) if np.ndim(win) == 0 else p(keep := to(np.ascontiguousarray(win, dtype=np.int32)))
    args = [p(Xa), snps, indiv, w, p(out)] + ([ldb] if "band" in entry else []) + [flag] + ([is_plink, p(fa)] if entry in PLAIN else [])
    rc = getattr(L, entry)(*args)
    if device:
        import torch
        torch.cuda.synchronize()
        out = out.cpu().numpy()
    assert (rc, L.mxa_last_error()) == (0, 0), (entry, mx.lib.last_error())
    assert np.all(out[nout:] == SENTINEL), entry
    return out[:nout]


def _band(mx, entry, X, snps, indiv, w, kind, f, device):
    """band entry with ldb = w + 4: (snps, w + 1) in-band part; zeros in the tail and the sentinel beyond the window are asserted here"""
    ldb = w + 4
    B = _call(mx, entry, X, snps, indiv, w, snps * ldb, kind, f, device, ldb=ldb).reshape(snps, ldb)
    inband = (np.arange(snps)[:, None] + np.arange(w + 1)[None, :]) < snps
    assert np.all(B[:, w + 1:] == SENTINEL), entry
    assert np.all(B[:, : w + 1][~inband] == 0.0) and not np.signbit(B[:, : w + 1][~inband]).any(), entry
    return B[:, : w + 1], inband


# ------------------------------------------------------------------------------------------------------------------ a. small and ragged shapes
_CASES = {}


def _edge_case(snps, indiv):
    """seeded binomial genotypes, every SNP polymorphic; f the data's own frequency; the pairwise data: the same with 10 % missing, where individuals 0, 1, 2 are
    always genotyped and carry 0, 2 at every SNP -- so every pair shares at least 3 individuals and no SNP is constant on a pair's shared ones, by construction"""
    key = (snps, indiv)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng([snps, indiv])
    Z = rng.binomial(2, rng.uniform(0.05, 0.95, size=snps)[:, None], size=(snps, indiv)).astype(np.int8)
    const = Z.min(axis=1) == Z.max(axis=1)
    Z[const, 0], Z[const, 1] = 0, 2
    X = np.ascontiguousarray(pack_plink(Z))
    f = Z.astype(np.float64).mean(axis=1) / 2.0
    c = dict(X=X, f=f, **ref.plain_case(X, indiv, f))
    assert np.all(c["sigma2"] > 0) and np.isfinite(c["b"]).all()
    Zp = Z.copy()
    Zp[:, 0], Zp[:, 1] = 0, 2
    miss = rng.random((snps, indiv)) < 0.10
    miss[:, :3] = False
    c["Xp"] = np.ascontiguousarray(pack_plink(Zp, miss))
    pw = ref.pairwise_restate(c["Xp"], indiv)
    assert pw["N"].min() >= 3 and np.isfinite(pw["r"]).all()
    c["rp"], c["bp"], c["gp"] = pw["r"], ref.pairwise_bound(pw["r"]), 1.0 / (pw["N"].astype(np.float64) - 2.0)
    c["seen"], c["worst"], c["sref"] = {}, {}, {}
    _CASES[key] = c
    return c


def _edge_windows(snps):
    """(name, last, fixed window or None)"""
    out = [(f"w={w}", ref.fixed_last(snps, w), w) for w in sorted({w for w in (0, 1, 31, 32, 33, snps - 1) if w < snps})]
    cut = snps // 2                                                             # two chromosomes: SNPs [0, cut) and [cut, snps), each one whole window
    if cut >= 1:
        out.append(("two chromosomes", np.where(np.arange(snps) < cut, cut - 1, snps - 1).astype(np.int32), None))
    return out


def _note(c, what, ratio):
    c["worst"][what] = max(c["worst"].get(what, 0.0), ratio)


def _same_bits(c, key, got):
    """the first configuration's result is kept; every other engine / pointer kind must give the same bits"""
    first = c["seen"].setdefault(key, got)
    assert np.array_equal(got, first), key


@pytest.mark.parametrize("snps,indiv", EDGE_SHAPES)
@pytest.mark.parametrize("engine", ["f4", "i8"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_all_entries_at_small_and_ragged_shapes(mx, monkeypatch, snps, indiv, engine, device):
    c = _edge_case(snps, indiv)
    monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
    X, f, Xp = c["X"], c["f"], c["Xp"]
    g = 1.0 / (indiv - 2.0)
    for name, last, w in _edge_windows(snps):
        ii, jj = ref.pairs(last)
        for route, Xr, fr, r, b, gg in (("", X, f, c["r"], c["b"], g), ("_pairwise", Xp, None, c["rp"], c["bp"], c["gp"])):
            rows = {}
            for kind in (0, 1):
                rows[kind] = _call(mx, "mxa_ld_window_rows" + route, Xr, snps, indiv, last, len(ii), kind, fr, device)
                _same_bits(c, ("rows" + route, name, kind), rows[kind])
            _note(c, "rows" + route, q := ref.worst_ratio(rows[0], r[ii, jj], b[ii, jj]))
            assert q <= 1.0, (route, name, q)
            assert np.array_equal(rows[1], rows[0] * rows[0]), (route, name)                       # r * r, one rounding
            for adjust in (0, 1):
                S = _call(mx, "mxa_ld_window_scores" + route, Xr, snps, indiv, last, snps, adjust, fr, device)
                _same_bits(c, ("wscores" + route, name, adjust), S)
                if (route, name, adjust) not in c["sref"]:                                          # the reference: once per shape, shared by the four configurations
                    c["sref"][route, name, adjust] = ref.scores_ref(r, b, gg if adjust else 0.0, last)
                want, tol = c["sref"][route, name, adjust]
                _note(c, "scores" + route, q := float((np.abs(S - want) / tol).max()))
                assert np.isfinite(S).all() and q <= 1.0, (route, name, adjust, q)
                if w is not None:                                                                  # the fixed entry: the same window, the same bits
                    S2 = _call(mx, "mxa_ld_scores" + route, Xr, snps, indiv, w, snps, adjust, fr, device)
                    assert np.array_equal(S2, S), (route, name, adjust)
            if w is not None:
                for kind in (0, 1):
                    B, inband = _band(mx, "mxa_ld_band" + route, Xr, snps, indiv, w, kind, fr, device)
                    assert np.array_equal(B[ii, jj - ii], rows[kind]) and int(inband.sum()) == len(ii), (route, name, kind)
    # mxa_ld of the same input: within the element bound, and its band is the band entries' bits
    R = mx.crossproduct.ld(X, snps, indiv, is_plink_format=True, allele_freq=f)
    _note(c, "mxa_ld", q := ref.worst_ratio(R, c["r"], c["b"]))
    assert q <= 1.0 and np.array_equal(R, R.T), q
    ii, jj = ref.pairs(ref.fixed_last(snps, snps - 1))
    assert np.array_equal(R[ii, jj], c["seen"]["rows", f"w={snps - 1}", 0])
    print(f"edges {snps}x{indiv} {engine} {'device' if device else 'host'}: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(c["worst"].items())))


# --------------------------------------------------------------------------------------------------------------- b. window geometry sweep
SWEEP_SNPS, SWEEP_INDIV = 700, 70


@pytest.fixture(scope="module")
def sweep(mx):
    """one problem for all 32 windows; mxa_ld's R of it, computed once and read-only"""
    c = dict(_edge_case(SWEEP_SNPS, SWEEP_INDIV))
    R = mx.crossproduct.ld(c["X"], SWEEP_SNPS, SWEEP_INDIV, is_plink_format=True, allele_freq=c["f"])
    R.setflags(write=False)
    c["R"] = R
    return c


@pytest.mark.parametrize("seed", range(32))
def test_seeded_window_geometries(mx, monkeypatch, sweep, seed):
    snps, indiv, c = SWEEP_SNPS, SWEEP_INDIV, sweep
    engine, device = ("f4", "i8")[seed & 1], bool(seed & 2)                     # alternate with the seed
    monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
    last = ref.sweep_window(snps, seed)
    ii, jj = ref.pairs(last)
    assert len(ii) == ref.rowptr_of(last)[-1]
    reach = int((last - np.arange(snps)).max())
    worst = {}
    for route, Xr, fr, r, b, gg in (("", c["X"], c["f"], c["r"], c["b"], 1.0 / (indiv - 2.0)), ("_pairwise", c["Xp"], None, c["rp"], c["bp"], c["gp"])):
        rows = [_call(mx, "mxa_ld_window_rows" + route, Xr, snps, indiv, last, len(ii), kind, fr, device) for kind in (0, 1)]
        worst["rows" + route] = ref.worst_ratio(rows[0], r[ii, jj], b[ii, jj])
        assert worst["rows" + route] <= 1.0, (route, worst)
        assert np.array_equal(rows[1], rows[0] * rows[0]), route
        if route == "":
            assert np.array_equal(rows[0], c["R"][ii, jj])                                         # mxa_ld's R bit for bit
        else:
            B = mx.crossproduct.ld_band_pairwise(Xr, snps, indiv, reach)                           # the r of a pair does not depend on the window
            assert np.array_equal(rows[0], B[ii, jj - ii])
        for adjust in (0, 1):
            S = _call(mx, "mxa_ld_window_scores" + route, Xr, snps, indiv, last, snps, adjust, fr, device)
            want, tol = ref.scores_ref(r, b, gg if adjust else 0.0, last)
            q = float((np.abs(S - want) / tol).max())
            worst["scores" + route] = max(worst.get("scores" + route, 0.0), q)
            assert np.isfinite(S).all() and q <= 1.0, (route, adjust, q)
    print(f"sweep seed {seed} {engine} {'device' if device else 'host'} reach 0 .. {reach}: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


# ------------------------------------------------------------------------------------------- c. the engine rule at its boundary, windowed routes
# FP4 is exact while sum z z' < 2^24: top^2 indiv < 2^24 with top = the largest staged value (2; 3 where the byte table turned a byte with a missing pair
# into four 3s).  The rule stands three times in the library (crossproduct, windowed LD, pairwise windowed LD); here the two windowed copies run just below
# and just above it, on rows that keep the fp32 accumulator at the top of its 24 bits when single quarter units arrive.
LIMIT_SNPS, LIMIT_CUT = 260, 130
LIMIT_ONES = (8, 4, 12, 100_000)                # SNP a: the largest value throughout, genotype 1 in the last LIMIT_ONES[a] individuals
LIMIT_BLOCK = np.array([0, 1, 2, 3] + list(range(7, 256, 13)) + [256, 257, 258, 259])      # the structured SNPs and 24 random ones, the second tile row included
LIMIT_CASES = [("clean", 4_194_300, 2, True), ("clean", 4_194_304, 2, False), ("missing", 4_194_300, 2, True), ("missing", 4_194_304, 2, False),
               ("threes", 1_864_132, 3, True), ("threes", 1_864_136, 3, False)]


def _limit_operand(data, indiv):
    """(packed matrix on the device, f = half the mean of the staged values as numpy) -- built on the device with torch"""
    import torch
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(indiv + len(data))
    snps = LIMIT_SNPS
    code = torch.randint(0, 3, (snps, indiv), generator=gen, device=dev, dtype=torch.uint8)
    code = torch.where(code == 0, code, code + 1)                                           # genotypes 0, 1, 2 -> PLINK codes 00, 10, 11
    if data in ("missing", "threes"):
        code[torch.randint(0, 20, (snps, indiv), generator=gen, device=dev, dtype=torch.uint8) == 0] = 1      # 5 % missing
    for a, ones in enumerate(LIMIT_ONES):
        code[a] = 1 if data == "threes" else 3                                              # a missing code in every byte: four 3s under the byte table
        code[a, indiv - ones:] = 2
    c4 = code.view(snps, indiv // 4, 4)
    X = (c4[:, :, 0] | (c4[:, :, 1] << 2) | (c4[:, :, 2] << 4) | (c4[:, :, 3] << 6)).contiguous()
    val = torch.where(c4 >= 2, c4 - 1, torch.zeros_like(c4))
    val = torch.where((c4 == 1).any(dim=2, keepdim=True), torch.full_like(c4, 3), val)      # the staged values of the plain route
    f = val.sum(dim=(1, 2), dtype=torch.int64).cpu().numpy() / (2.0 * indiv)
    return X, f


@pytest.mark.parametrize("data,indiv,top,below", LIMIT_CASES)
def test_engine_rule_at_its_boundary_on_the_windowed_routes(mx, monkeypatch, data, indiv, top, below):
    import torch
    assert (top * top * indiv < 2 ** 24) == below and indiv % 4 == 0
    snps, w = LIMIT_SNPS, LIMIT_SNPS - 1
    Xd, f = _limit_operand(data, indiv)
    host = data == "clean" and below                    # 260 x 1 048 575 bytes from the host: 273 MB, two staging chunks of the 256 MiB bounce buffer
    assert not host or snps * (indiv // 4) > (256 << 20) > 256 * (indiv // 4)
    X = Xd.cpu().numpy() if host else Xd
    fd = f if host else torch.from_numpy(f).to(Xd.device)
    last = np.where(np.arange(snps) < LIMIT_CUT, LIMIT_CUT - 1, snps - 1).astype(np.int32)
    ii, jj = ref.pairs(last)
    lastd = last if host else torch.from_numpy(last).to(Xd.device)
    cp = mx.crossproduct
    to_np = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()
    routes = (["plain"] if data != "missing" else []) + (["pairwise"] if data != "threes" else [])
    blk = LIMIT_BLOCK
    Xb = Xd[torch.from_numpy(blk).to(Xd.device)].cpu().numpy()                              # the 28 rows of the block, for the reference
    lo, hi = np.minimum.outer(LIMIT_ONES, LIMIT_ONES), np.maximum.outer(LIMIT_ONES, LIMIT_ONES)
    closed = top * top * (indiv - hi) + top * (hi - lo) + lo                                # M_ij of the structured pairs
    worst = {}
    for route in routes:
        got = {}
        for engine in (None, "i8"):
            if engine is None:
                monkeypatch.delenv("MXA_XPROD_ENGINE", raising=False)
            else:
                monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
            if route == "plain":
                res = (cp.ld_band(X, snps, indiv, w, is_plink_format=True, allele_freq=fd),
                       cp.ld_window_rows(X, snps, indiv, lastd, is_plink_format=True, allele_freq=fd),
                       cp.ld_window_scores(X, snps, indiv, lastd, adjust=True, is_plink_format=True, allele_freq=fd))
            else:
                res = (cp.ld_band_pairwise(X, snps, indiv, w), cp.ld_window_rows_pairwise(X, snps, indiv, lastd),
                       cp.ld_window_scores_pairwise(X, snps, indiv, lastd, adjust=True))
            got[engine] = [to_np(a) for a in res]
        for a, b in zip(got[None], got["i8"]):
            assert np.isfinite(a).all() and np.array_equal(a, b), (route, "the default engine and int8 differ")
        band, rows, _ = got[None]
        assert np.array_equal(band[ii, jj - ii], rows), route                               # the band equals the rows where both exist
        # the 28 x 28 block against the definition, the reference in K chunks
        if route == "plain":
            M = ref.gram_exact(ref.staged(Xb))
            r, b = ref.ld_ref(M, f[blk], indiv)
        else:
            pw = ref.pairwise_restate(Xb, indiv, check_rows=2)
            M, r, b = pw["Sxy"].astype(np.float64), pw["r"], ref.pairwise_bound(pw["r"])
            assert pw["N"][:4, :4].min() == indiv
        assert np.array_equal(M[:4, :4], closed.astype(np.float64)), route
        bi, bj = np.meshgrid(blk, blk, indexing="ij")
        up = bi <= bj
        worst[route] = ref.worst_ratio(band[bi[up], (bj - bi)[up]], r[up], b[up])
        assert np.isfinite(b).all() and worst[route] <= 1.0, (route, worst)
    print(f"engine rule {data} indiv={indiv} ({'below' if below else 'above'}, {'host' if host else 'device'} operand): worst |err| / bound "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------------- d. more than 2^31 stored entries
def test_more_than_two_to_the_31_stored_entries(mx):
    """rowptr[] and the band index gi * ldb are 64-bit: 100 000 SNPs with a reach of 32 767 store 2 739 945 472 entries (21.9 GB) as ragged rows and
    100 000 x 32 768 (26.2 GB) as a band; device-resident"""
    import torch
    if torch.cuda.mem_get_info()[0] < 40 * 10 ** 9:
        pytest.skip("needs 40 GB of free device memory")
    dev = torch.device("cuda", 0)
    from _ld_limits_ref import big_window_problem
    P = big_window_problem()                                # the generator, shared with tests/test_ld_limits_gpu.py
    snps, indiv, w, rng, X, Zl, f, diag = P["snps"], P["indiv"], P["w"], P["rng"], P["X"], P["Zl"], P["f"], P["diag"]
    last, total, k, si, sj = P["last"], P["total"], P["k"], P["si"], P["sj"]
    r, b = ref.ld_ref_pairs((Zl[si] * Zl[sj]).sum(axis=1), diag[si], diag[sj], f[si], f[sj], indiv)
    Xd, fd, lastd = torch.from_numpy(X).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(last).to(dev)
    L = mx.lib.check_library_handle()
    p = mx.lib.ptr
    out = torch.full((total + PAD,), SENTINEL, dtype=torch.float64, device=dev)
    assert L.mxa_ld_window_rows(p(Xd), snps, indiv, p(lastd), p(out), 0, 1, p(fd)) == 0, mx.lib.last_error()
    torch.cuda.synchronize()
    assert int((out != SENTINEL).sum()) == total and bool((out[total:] == SENTINEL).all())
    rows = out[torch.from_numpy(k).to(dev)].cpu().numpy()
    del out
    torch.cuda.empty_cache()
    q_rows = ref.worst_ratio(rows, r, b)
    assert q_rows <= 1.0, q_rows
    ldb = w + 1
    band = torch.full((snps * ldb + PAD,), SENTINEL, dtype=torch.float64, device=dev)
    assert L.mxa_ld_band(p(Xd), snps, indiv, w, p(band), ldb, 0, 1, p(fd)) == 0, mx.lib.last_error()
    torch.cuda.synchronize()
    kb = si.astype(np.int64) * ldb + (sj - si)
    assert kb.max() > 2 ** 31 and bool((band[snps * ldb:] == SENTINEL).all())
    assert np.array_equal(band[torch.from_numpy(kb).to(dev)].cpu().numpy(), rows)           # band and rows: the same bits
    del band
    torch.cuda.empty_cache()
    # scores at 32 SNPs, first and last included
    S = mx.crossproduct.ld_window_scores(Xd, snps, indiv, lastd, adjust=True, is_plink_format=True, allele_freq=fd).cpu().numpy()
    first = ref.first_of(last)
    q_scores = 0.0
    for i in np.concatenate([[0, snps - 1], rng.integers(1, snps - 1, size=30)]):
        j = np.arange(first[i], last[i] + 1)
        ri, bi = ref.ld_ref_pairs(Zl[j] @ Zl[i], diag[i], diag[j], f[i], f[j], indiv)
        want, tol = ref.score_row(ri, bi, 1.0 / (indiv - 2.0))
        q_scores = max(q_scores, abs(S[i] - want) / tol)
    print(f"2^31 entries: {total} stored, worst |err| / bound rows {q_rows:.3f}, scores {q_scores:.2e} (up to 65 535 terms)")
    assert np.isfinite(S).all() and q_scores <= 1.0, q_scores
