"""mxa_ld_prune_csr / mxa_ld_window_prune / mxa_ld_window_prune_pairwise without a device: the three symbols in every layer that names the C ABI with the
prototypes of the header, the argument errors decided before a device is selected, the Python argument checks (raised before any library call), and the
reference walk of the GPU tests (tests/_ld_prune_ref.py) against the brute-force definition: the lexicographically first maximal independent set."""
import ctypes
import fnmatch
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from _ld_prune_ref import csr_of_edges, order_of, ref_greedy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mxa_ld_prune_csr", "mxa_ld_window_prune", "mxa_ld_window_prune_pairwise")
SNPS, INDIV = 5, 8
SENT_L, SENT_I, SENT_B, SENT_R = -7_777_777_777, -777_777, 0xAB, -777
CTYPE = {"int": ctypes.c_int, "double": ctypes.c_double, "long *": ctypes.POINTER(ctypes.c_long), "int *": ctypes.POINTER(ctypes.c_int)}


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _header_prototype(sym):
    """[(type, name)] of the header's declaration"""
    header = re.sub(r"/\*.*?\*/", "", _read("include", "miraculix_amd.h"), flags=re.S)
    args = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % sym, header).group(1)
    out = []
    for a in args.split(","):
        t, name = re.match(r"\s*(.*?)(\w+)\s*$", a, flags=re.S).groups()
        out.append((" ".join(t.replace("*", " * ").split()), name))
    return out


def test_the_three_symbols_are_in_every_layer_with_the_headers_prototypes(mx):
    fortran = _read("miraculix_amd", "bindings", "fortran", "modmiraculix_amd.f90")
    public = " ".join(re.findall(r"^\s*public\s*::(.*)$", fortran, flags=re.M))
    patterns = re.findall(r"([\w*]+)\s*;", re.sub(r"/\*.*?\*/", "", _read("miraculix_amd", "csrc", "exports.map"), flags=re.S).split("local:")[0])
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "miraculix_amd", "lib", "libmiraculix_amd.so")],
                                                                 text=True).splitlines() if ln.strip()}
    L = mx.lib.check_library_handle()
    want = {"mxa_ld_prune_csr": "snps rowptr col priority keep owner n_kept rounds",
            "mxa_ld_window_prune": "plink snps indiv last min_r2 priority keep owner n_kept rounds is_plink_format allele_freq",
            "mxa_ld_window_prune_pairwise": "plink snps indiv last min_r2 priority keep owner n_kept rounds"}
    for sym in SYMBOLS:
        proto = _header_prototype(sym)
        assert [n for _, n in proto] == want[sym].split(), sym
        assert dict((n, t) for t, n in proto)["n_kept"] == "long *" and dict((n, t) for t, n in proto)["keep"] == "unsigned char *", sym
        assert any(fnmatch.fnmatchcase(sym, p) for p in patterns) and sym in exported, sym       # global in the version script, and in the dynamic symbol table
        fn = getattr(L, sym)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None and len(fn.argtypes) == len(proto), sym
        for (t, name), at in zip(proto, fn.argtypes):                                              # host-only pointers typed, every other pointer void *
            assert at is (CTYPE[t] if name in ("n_kept", "rounds") or "*" not in t else ctypes.c_void_p), (sym, name, t, at)
        assert re.search(r"bind\(C,\s*name='%s'\)" % sym, fortran) and re.search(r"\b%s\b" % sym, public), sym
    comment = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mxa_ld_prune_csr\(", _read("include", "miraculix_amd.h"), flags=re.S).group(1)
    assert "unique" in comment and "do not depend on the engine" in comment                         # the definition, with the uniqueness statement
    assert int(re.search(r"\((\d+) C symbols", _read("README.md")).group(1)) == len(exported)         # the README's symbol-count line


def _valid():
    """arguments that only a device could still refuse, outputs filled with sentinels"""
    return dict(plink=np.zeros((SNPS, (INDIV + 3) // 4), np.uint8), snps=SNPS, indiv=INDIV, last=np.full(SNPS, SNPS - 1, np.int32), min_r2=0.2, priority=None,
                keep=np.full(SNPS, SENT_B, np.uint8), owner=np.full(SNPS, SENT_I, np.int32), n_kept=ctypes.c_long(SENT_L), rounds=ctypes.c_int(SENT_R),
                freq=np.full(SNPS, 0.25), rowptr=np.array([0, 1, 1, 1, 1, 1], np.int64), col=np.array([1], np.int32))


BAD = [("keep NULL", dict(keep=None)), ("n_kept NULL", dict(n_kept=None)), ("snps 0", dict(snps=0)), ("snps negative", dict(snps=-3))]


@pytest.mark.parametrize("entry", SYMBOLS)
@pytest.mark.parametrize("what,change", BAD, ids=[b[0] for b in BAD])
def test_argument_errors_before_a_device_is_selected(mx, entry, what, change):
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    a = _valid()
    held = dict(a)                                                                                  # the arrays themselves: checked after the call
    a.update(change)
    n_kept = None if a["n_kept"] is None else ctypes.byref(a["n_kept"])
    outs = [p(a["priority"]), p(a["keep"]), p(a["owner"]), n_kept, ctypes.byref(a["rounds"])]
    if entry == "mxa_ld_prune_csr":
        rc = L.mxa_ld_prune_csr(a["snps"], p(a["rowptr"]), p(a["col"]), *outs)
    else:
        args = [p(a["plink"]), a["snps"], a["indiv"], p(a["last"]), a["min_r2"]] + outs
        rc = getattr(L, entry)(*(args + ([1, p(a["freq"])] if entry == "mxa_ld_window_prune" else [])))
    assert (rc, L.mxa_last_error()) == (1, 1), (what, mx.lib.last_error())
    assert np.all(held["keep"] == SENT_B) and np.all(held["owner"] == SENT_I) and held["n_kept"].value == SENT_L and held["rounds"].value == SENT_R, what


def test_python_argument_checks_raise_before_any_library_call(mx, monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(mx.lib, "check_library_handle", no_library)
    X, f = np.zeros((SNPS, (INDIV + 3) // 4), np.uint8), np.full(SNPS, 0.25)
    last = np.full(SNPS, SNPS - 1, np.int32)
    prune = mx.crossproduct.ld_prune
    for pairwise in (False, True):
        kw = dict(pairwise=pairwise, allele_freq=None if pairwise else f)
        for bad in (dict(), dict(last=last, window=2)):
            with pytest.raises(ValueError, match="exactly one of last and window"):
                prune(X, SNPS, INDIV, **kw, **bad)
        with pytest.raises(ValueError, match="Window needs to be in"):
            prune(X, SNPS, INDIV, window=SNPS, **kw)
        with pytest.raises(ValueError, match="last needs"):
            prune(X, SNPS, INDIV, last=last[::-1] - 1, **kw)
        with pytest.raises(ValueError, match="wrong dimensions"):
            prune(X[:-1], SNPS, INDIV, window=2, **kw)
        with pytest.raises(ValueError, match="priority must not hold a NaN"):
            prune(X, SNPS, INDIV, window=2, priority=np.array([0.1, np.nan, 0.3, 0.4, 0.5]), **kw)
        with pytest.raises(ValueError, match="priority needs to be 5 float64 values"):
            prune(X, SNPS, INDIV, window=2, priority=np.zeros(4), **kw)
    with pytest.raises(ValueError, match="Allele frequencies"):
        prune(X, SNPS, INDIV, window=2)
    with pytest.raises(ValueError, match="priority must not hold a NaN"):
        mx.ld_prune_csr(np.array([0, 1, 1], np.int64), np.array([1], np.int32), priority=np.array([np.nan, 1.0]))
    with pytest.raises(ValueError, match="priority needs to be 2 float64 values"):
        mx.ld_prune_csr(np.array([0, 1, 1], np.int64), np.array([1], np.int32), priority=np.zeros(3))
    with pytest.raises(ValueError, match="rowptr needs"):
        mx.ld_prune_csr(np.array([0], np.int64), np.array([], np.int32))


# ------------------------------------------------------------------------------------------------ the reference walk against the definition
def _brute_force(n, edges, priority):
    """the lexicographically first maximal independent set under the order, by enumeration: among all maximal independent sets, the one whose members, listed
    in the order, come first; and the owners from the definition (the first kept neighbour in the order)"""
    order = [int(v) for v in order_of(n, priority)]
    rank = {v: k for k, v in enumerate(order)}
    adj = [set() for _ in range(n)]
    for a, b in edges:
        adj[a].add(b)
        adj[b].add(a)
    best = None
    for bits in itertools.product((False, True), repeat=n):
        s = {v for v in range(n) if bits[v]}
        if any(adj[v] & s for v in s) or any(not (adj[v] & s) for v in range(n) if v not in s):
            continue                                                                                # not independent, or not maximal
        seq = sorted(rank[v] for v in s)
        if best is None or seq < best[0]:
            best = (seq, s)
    keep = np.array([v in best[1] for v in range(n)], dtype=bool)
    owner = np.array([v if keep[v] else min(adj[v] & best[1], key=rank.get) for v in range(n)], dtype=np.int32)
    return keep, owner


def test_the_reference_walk_is_the_lexicographically_first_maximal_independent_set():
    rng = np.random.default_rng(20240607)
    seen = set()
    for g in range(200):
        n = int(rng.integers(1, 13))
        density = rng.choice([0.0, 0.15, 0.4, 0.8, 1.0])
        edges = [(a, b) for a in range(n) for b in range(a + 1, n) if rng.random() < density]
        kind = g % 4
        priority = (None, rng.random(n), rng.integers(0, 3, size=n).astype(np.float64), rng.choice([-np.inf, -0.0, 0.0, 1.0, np.inf], size=n))[kind]
        rowptr, col = csr_of_edges(n, edges)
        keep, owner = ref_greedy(n, rowptr, col, priority)
        want_keep, want_owner = _brute_force(n, edges, priority)
        assert np.array_equal(keep, want_keep) and np.array_equal(owner, want_owner), (g, n, edges, priority)
        seen.add((n, kind))
    assert len(seen) >= 40                                                                          # every size under every kind of priority, nearly
