"""mxa_ld_window_pairs / mxa_ld_window_pairs_pairwise without a device: the two symbols in every layer that names the C ABI, and the argument errors that are
decided before a device is selected -- return 1, mxa_last_error() == 1, sentinel-filled outputs untouched."""
import ctypes
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mxa_ld_window_pairs", "mxa_ld_window_pairs_pairwise")
SNPS, INDIV, CAP = 5, 8, 16
SENT_L, SENT_I, SENT_D = -7_777_777_777, -777_777, -12345.678


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_both_symbols_are_in_every_layer(mx):
    header = re.sub(r"/\*.*?\*/", "", _read("include", "miraculix_amd.h"), flags=re.S)
    fortran = _read("miraculix_amd", "bindings", "fortran", "modmiraculix_amd.f90")
    public = " ".join(re.findall(r"^\s*public\s*::(.*)$", fortran, flags=re.M))
    patterns = re.findall(r"([\w*]+)\s*;", re.sub(r"/\*.*?\*/", "", _read("miraculix_amd", "csrc", "exports.map"), flags=re.S).split("local:")[0])
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "miraculix_amd", "lib", "libmiraculix_amd.so")],
                                                                 text=True).splitlines() if ln.strip()}
    L = mx.lib.check_library_handle()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert any(fnmatch.fnmatchcase(sym, p) for p in patterns) and sym in exported, sym       # global in the version script, and in the dynamic symbol table
        fn = getattr(L, sym)
        assert fn.argtypes is not None and len(fn.argtypes) == (13 if sym == SYMBOLS[0] else 11) and fn.restype is ctypes.c_int, sym
        assert fn.argtypes[4] is ctypes.c_double and fn.argtypes[9] is ctypes.c_long, sym
        assert re.search(r"bind\(C,\s*name='%s'\)" % sym, fortran) and re.search(r"\b%s\b" % sym, public), sym
    comment = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mxa_ld_window_pairs\(", _read("include", "miraculix_amd.h"), flags=re.S).group(1)
    assert "mxa_last_error() == 25" in comment                                                      # the definition, with the new error code


def _valid():
    """arguments of a filling call that only a device could still refuse, outputs filled with sentinels"""
    return dict(plink=np.zeros((SNPS, (INDIV + 3) // 4), np.uint8), snps=SNPS, indiv=INDIV, last=np.full(SNPS, SNPS - 1, np.int32), min_r2=0.2, kind=0,
                rowptr=np.full(SNPS + 1, SENT_L, np.int64), col=np.full(CAP, SENT_I, np.int32), val=np.full(CAP, SENT_D, np.float64), capacity=CAP,
                total=ctypes.c_long(SENT_L), freq=np.full(SNPS, 0.25))


BAD = [("rowptr NULL", dict(rowptr=None)), ("total NULL", dict(total=None)), ("col NULL only", dict(col=None)), ("val NULL only", dict(val=None)),
       ("min_r2 negative", dict(min_r2=-0.0001)), ("min_r2 NaN", dict(min_r2=float("nan"))), ("min_r2 inf", dict(min_r2=float("inf"))), ("kind 2", dict(kind=2)),
       ("snps 0", dict(snps=0)), ("snps negative", dict(snps=-3))]


@pytest.mark.parametrize("pairwise", [False, True], ids=["plain", "pairwise"])
@pytest.mark.parametrize("what,change", BAD, ids=[b[0] for b in BAD])
def test_argument_errors_before_a_device_is_selected(mx, pairwise, what, change):
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    a = _valid()
    keep = dict(a)                                                                                  # the arrays themselves: checked after the call
    a.update(change)
    total = a["total"]
    args = [p(a["plink"]), a["snps"], a["indiv"], p(a["last"]), a["min_r2"], a["kind"], p(a["rowptr"]), p(a["col"]), p(a["val"]), a["capacity"],
            None if total is None else ctypes.byref(total)]
    if not pairwise:
        args += [1, p(a["freq"])]
    rc = getattr(L, SYMBOLS[1] if pairwise else SYMBOLS[0])(*args)
    assert (rc, L.mxa_last_error()) == (1, 1), (what, mx.lib.last_error())
    assert np.all(keep["rowptr"] == SENT_L) and np.all(keep["col"] == SENT_I) and np.all(keep["val"] == SENT_D) and keep["total"].value == SENT_L, what


def test_python_wrapper_wants_exactly_one_of_last_and_window(mx):
    X, f = np.zeros((SNPS, (INDIV + 3) // 4), np.uint8), np.full(SNPS, 0.25)
    last = np.full(SNPS, SNPS - 1, np.int32)
    for kw in (dict(), dict(last=last, window=2)):
        for pairwise in (False, True):
            with pytest.raises(ValueError, match="exactly one of last and window"):
                mx.crossproduct.ld_pairs(X, SNPS, INDIV, pairwise=pairwise, allele_freq=None if pairwise else f, **kw)
