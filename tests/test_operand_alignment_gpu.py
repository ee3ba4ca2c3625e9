"""Every pointer argument of the C ABI is valid at its element type's natural alignment, in host or device memory, and the results do not depend on it
(include/miraculix_amd.h).  The generators of the suite hand over the base of a fresh allocation every time (64 bytes for numpy, 256 for torch); a caller
hands over base + 3 of a memory-mapped .bed, a torch slice, a column of a bigger buffer, a Fortran array section.  The kernels choose code paths by the
address: dword or byte-wise loads of packed rows (k_recode, the crossproduct staging), the tiled or the generic 2-bit transpose, the 16-byte head of the
frequency count, one 16-byte or two 8-byte stores of a product's result.

Each case: the entry through the raw ctypes handle with ONE operand (or one pair) moved by `elems` elements past a 64-byte boundary -- packed bytes and keep[]
by 1, 2, 3, 5 bytes; ints by 1, 2, 3 (4, 8, 12 mod 16); doubles and longs by 1 (8 mod 16) -- against the call with every operand on a 64-byte boundary:
the same bits in every output, and the guards of 64 bytes in front of and behind every output intact.  Host and device memory."""
import ctypes

import numpy as np
import pytest

import _ld_ref as ref
import _operands as ops
from _util import make_B, make_problem, random_csr

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
MIN_R2 = 0.002                           # about a third of the pairs of 526 individuals
GUARD_BYTES = 64
GUARDS = {np.dtype(np.float64): SENTINEL, np.dtype(np.int64): -7, np.dtype(np.int32): -7, np.dtype(np.uint8): 0xA5}


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    m.dgemm_compressed.set_options(use_gpu=True, not_center=False, verbose=0)
    return m


@pytest.fixture(autouse=True)
def _default_environment(monkeypatch):
    for name in ("MXA_XPROD_ENGINE", "MXA_XPROD_FUSED_POST", "MIRACULIX_NUM_GPUS", "MXA_LD_PAIRWISE_SCRATCH_MB", "MXA_LD_PAIRWISE_DENSE"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("MXA_SINGLE_ORIENTATION", "0")                # objects keep both packed copies: plink_transposed is read


# --------------------------------------------------------------------------------------------------------------------------------------- tools
class Place:
    """where the operands of one call lie: every operand `shift` does not name on a 64-byte boundary, the named ones `elems` elements behind one"""

    def __init__(self, device=False, shift=None):
        self.device, self.shift, self.held, self.outs = device, dict(shift or {}), [], []
        self.used = set()

    def inp(self, name, a, device=None):
        if a is None:
            return None
        arr, addr = ops.misaligned(a, self.shift.get(name, 0), self.device if device is None else device)
        self.held.append(arr)
        self.used.add(name)
        return ctypes.c_void_p(addr)

    def out(self, name, init, device=None):
        """an output that starts as `init` (sentinels), with 64 bytes of guard elements on either side"""
        init = np.ascontiguousarray(init)
        g = GUARD_BYTES // init.dtype.itemsize
        guard = np.full(g, GUARDS[init.dtype], init.dtype)
        arr, addr = ops.misaligned(np.concatenate([guard, init.reshape(-1), guard]), self.shift.get(name, 0), self.device if device is None else device)
        self.outs.append((name, arr, g, init.shape))
        self.used.add(name)
        return ctypes.c_void_p(addr + GUARD_BYTES)

    def results(self):
        assert set(self.shift) <= self.used, (self.shift, self.used)   # a name that matches no operand would test nothing
        res = []
        for name, arr, g, shape in self.outs:
            if hasattr(arr, "detach"):
                import torch
                torch.cuda.synchronize()
            flat = ops.readback(arr)
            assert np.all(flat[:g] == GUARDS[flat.dtype]) and np.all(flat[-g:] == GUARDS[flat.dtype]), ("written outside", name)
            res.append(flat[g:-g].reshape(shape))
        return res


def _same(got, want, what):
    assert len(got) == len(want), what
    for q, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, q)
        assert np.array_equal(ops.bits(g), ops.bits(w)), (what, q, int((ops.bits(g) != ops.bits(w)).sum()))


def _sweep(fn, shifts, devices=(False, True)):
    """fn(Place) -> outputs, for every (names, offsets) of `shifts` ("a+b": both operands moved) against the aligned call, on the host and on the device"""
    for device in devices:
        base = fn(Place(device))
        assert all(np.size(b) > 0 for b in base)
        for names, offsets in shifts.items():
            for off in offsets:
                _same(fn(Place(device, {n: off for n in names.split("+")})), base, ("device" if device else "host", names, off))


_PROBLEMS = {}


def _problem(snps, indiv, missing_frac):
    key = (snps, indiv, missing_frac)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = make_problem(snps, indiv, 1, seed=snps + indiv, missing_frac=missing_frac)
    return _PROBLEMS[key]


def _ok(mx, rc=0):
    L = mx.lib.check_library_handle()
    assert rc == 0 and L.mxa_last_error() == 0, mx.lib.last_error()


def _object(mx, pl, prob, one_pointer=False):
    L = mx.lib.check_library_handle()
    h = ctypes.c_void_p(None)
    L.plink2compressed(pl.inp("plink", prob["plink"]), None if one_pointer else pl.inp("plink_t", prob["plink_t"]), prob["snps"], prob["indiv"],
                       pl.inp("f", prob["f"]), 3, ctypes.byref(h))
    assert h.value, mx.lib.last_error()
    return h


def _both_products(mx, pl, h, snps, indiv, n=3):
    """'N' and 'T' with n columns into guarded outputs, and the stored frequencies"""
    L = mx.lib.check_library_handle()
    for t in (0, 1):
        k, m = (indiv, snps) if t else (snps, indiv)
        L.dgemm_compressed(b"T" if t else b"N", h, n, pl.inp("B", make_B(k, n, seed=3 + t)), k, pl.out("C", np.full((n, m), SENTINEL)), m)
        _ok(mx)
    L.get_compressed_freq(h, pl.out("f out", np.full(snps, SENTINEL), device=False))


# --------------------------------------------------------------------------------------------------------------------------- 1. packed inputs
@pytest.mark.parametrize("snps,indiv", ops.ALIGNMENT_SHAPES)
def test_packed_inputs_of_the_objects_at_byte_offsets(mx, snps, indiv):
    prob = _problem(snps, indiv, 0.05)
    L = mx.lib.check_library_handle()

    def two_pointers(pl):
        h = _object(mx, pl, prob)
        try:
            _both_products(mx, pl, h, snps, indiv)
        finally:
            L.free_compressed(ctypes.byref(h))
        return pl.results()

    def one_pointer(pl):
        h = _object(mx, pl, prob, one_pointer=True)
        try:
            _both_products(mx, pl, h, snps, indiv)
        finally:
            L.free_compressed(ctypes.byref(h))
        return pl.results()

    def rows(pl):
        h = ctypes.c_void_p(None)
        _ok(mx, L.mxa_plink2compressed_begin(snps, indiv, 3, ctypes.byref(h)))
        try:
            cut = 32 if snps < 128 else 128
            for b, e in ((cut, snps), (0, cut)):                      # the frequencies are counted on the device from the same rows
                _ok(mx, L.mxa_plink2compressed_rows(h, pl.inp("rows", prob["plink"][b:e]), b, e - b, None))
            _ok(mx, L.mxa_plink2compressed_end(h))
            _both_products(mx, pl, h, snps, indiv)
        finally:
            L.free_compressed(ctypes.byref(h))
        return pl.results()

    B = ops.BYTE_OFFSETS
    _sweep(two_pointers, {"plink": B, "plink_t": B, "plink+plink_t": B, "f": ops.WIDE_OFFSETS})
    _sweep(one_pointer, {"plink": B})
    _sweep(rows, {"rows": B})


@pytest.mark.parametrize("snps,indiv", ops.ALIGNMENT_SHAPES)
def test_packed_inputs_of_the_staging_helpers_and_one_call_products_at_byte_offsets(mx, snps, indiv):
    prob = _problem(snps, indiv, 0.05)
    P, Pt, f = prob["plink"], prob["plink_t"], prob["f"]
    L = mx.lib.check_library_handle()
    csr = {tc: random_csr(9, indiv if tc else snps, 12, seed=3 + tc) for tc in (0, 1)}

    def transpose(pl):
        _ok(mx, L.mxa_transpose_2bit(pl.inp("in", P), snps, indiv, pl.out("out", np.full(Pt.shape, 0x5A, np.uint8))))
        _ok(mx, L.mxa_transpose_2bit(pl.inp("in", Pt), indiv, snps, pl.out("out", np.full(P.shape, 0x5A, np.uint8))))
        res = pl.results()
        assert np.array_equal(res[0], Pt) and np.array_equal(res[1], P)
        return res

    def freq(pl):
        _ok(mx, L.mxa_allele_freq(pl.inp("plink", P), snps, indiv, pl.out("f", np.full(snps, SENTINEL))))
        _ok(mx, L.mxa_allele_freq(pl.inp("plink", Pt), indiv, snps, pl.out("f", np.full(indiv, SENTINEL))))
        return pl.results()

    def sparse(pl):
        for tc in (0, 1):
            ia, ja, a = csr[tc]
            entries = snps if tc else indiv
            L.sparse_times_plink(b"N", b"T" if tc else b"N", None if tc else pl.inp("plink", P), pl.inp("plink", Pt) if tc else None, snps, indiv, 9,
                                 pl.inp("I", ia), pl.inp("J", ja), pl.inp("B", a), pl.out("C", np.full((entries, 11), SENTINEL)), 11)
            _ok(mx)
        return pl.results()

    def dgemm_plink(pl):
        for t in (0, 1):
            k, m = (indiv, snps) if t else (snps, indiv)
            for freq_ in (f, None):
                L.dgemm_plink(b"T" if t else b"N", pl.inp("plink", P) if t else None, None if t else pl.inp("plink", Pt), snps, indiv, pl.inp("f", freq_), 3,
                              pl.inp("B", make_B(k, 3, seed=5 + t)), k, pl.out("C", np.full((3, m), SENTINEL)), m)
                _ok(mx)
        return pl.results()

    def crossproduct(pl):
        for X, k, rows in ((Pt, snps, indiv), (P, indiv, snps)):
            _ok(mx, L.snp_multiply_gpu(pl.inp("X", X), k, rows, pl.out("ans", np.full((rows, rows), SENTINEL)), True))
        return pl.results()

    B, W, I = ops.BYTE_OFFSETS, ops.WIDE_OFFSETS, ops.INT_OFFSETS
    _sweep(transpose, {"in": B, "out": B, "in+out": B})
    _sweep(freq, {"plink": B, "f": W})
    _sweep(sparse, {"plink": B, "I": I, "J": I, "B": W, "C": W})
    _sweep(dgemm_plink, {"plink": B, "f": W, "B": W, "C": W})
    _sweep(crossproduct, {"X": B, "ans": W})


@pytest.mark.parametrize("snps,indiv", ops.ALIGNMENT_SHAPES)
def test_packed_inputs_of_the_windowed_ld_entries_at_byte_offsets(mx, snps, indiv):
    plain, miss = _problem(snps, indiv, 0.0), _problem(snps, indiv, 0.05)
    L = mx.lib.check_library_handle()
    last = ref.fixed_last(snps, 40)
    total = int(ref.rowptr_of(last)[-1])

    def rows_plain(pl):
        _ok(mx, L.mxa_ld_window_rows(pl.inp("plink", plain["plink"]), snps, indiv, pl.inp("last", last), pl.out("rows", np.full(total, SENTINEL)), 0, 1,
                                     pl.inp("f", plain["f"])))
        res = pl.results()
        assert np.isfinite(res[0]).all()
        return res

    def scores_pairwise(pl):
        _ok(mx, L.mxa_ld_window_scores_pairwise(pl.inp("plink", miss["plink"]), snps, indiv, pl.inp("last", last), pl.out("scores", np.full(snps, SENTINEL)), 1))
        _ok(mx, L.mxa_ld_window_rows_pairwise(pl.inp("plink", miss["plink"]), snps, indiv, pl.inp("last", last), pl.out("rows", np.full(total, SENTINEL)), 0))
        return pl.results()

    B, W, I = ops.BYTE_OFFSETS, ops.WIDE_OFFSETS, ops.INT_OFFSETS
    _sweep(rows_plain, {"plink": B, "last": I, "f": W, "rows": W})
    _sweep(scores_pairwise, {"plink": B, "last": I, "scores": W, "rows": W})


# ------------------------------------------------------------------------------------------------------------------- 2. doubles at 8 mod 16
@pytest.mark.parametrize("snps,indiv", [(1200, 333), (333, 2)])
def test_b_and_c_of_the_products_at_8_mod_16(mx, snps, indiv):
    """m in {2, 333, 1200} (m = indiv for 'N', snps for 'T'), n in {1, 3, 8, 33}, even and odd leading dimensions: k_finish stores 16 bytes where C's column
    allows it and two doubles where not; the B packers read the caller's columns where they lie"""
    prob = _problem(snps, indiv, 0.05)
    L = mx.lib.check_library_handle()
    h = _object(mx, Place(), prob)
    try:
        for t in (0, 1):
            k, m = (indiv, snps) if t else (snps, indiv)
            for n in (1, 3, 8, 33):
                Bm = make_B(k, n, seed=7 + n + t)
                for pad in (0, 1):                                    # one of the two parities of ldb and of ldc each
                    ldb, ldc = k + pad, m + pad + 2 * (n % 2)

                    def product(pl):
                        Bp = np.full((n, ldb), 1e300)
                        Bp[:, :k] = Bm
                        b, c = pl.inp("B", Bp), pl.out("C", np.full((n, ldc), SENTINEL))
                        if pl.device:
                            _ok(mx, L.mxa_dgemm_compressed_device(b"T" if t else b"N", h, n, b, ldb, c, ldc, None, 1))
                        else:
                            L.dgemm_compressed(b"T" if t else b"N", h, n, b, ldb, c, ldc)
                            _ok(mx)
                        res = pl.results()
                        assert np.isfinite(res[0][:, :m]).all() and (pl.device or np.all(res[0][:, m:] == 0.0))
                        return res

                    _sweep(product, {"B": ops.WIDE_OFFSETS, "C": ops.WIDE_OFFSETS, "B+C": ops.WIDE_OFFSETS})
        if indiv > 2:
            def gram(pl):
                v, o = pl.inp("V", make_B(indiv, 3, seed=2, ldb=indiv + 1)), pl.out("out", np.full((3, indiv + 1), SENTINEL))
                if pl.device:
                    _ok(mx, L.mxa_gram_matvec_device(h, 3, v, indiv + 1, o, indiv + 1, 1))
                else:
                    _ok(mx, L.mxa_gram_matvec(h, 3, v, indiv + 1, o, indiv + 1))
                return pl.results()

            _sweep(gram, {"V": ops.WIDE_OFFSETS, "out": ops.WIDE_OFFSETS, "V+out": ops.WIDE_OFFSETS})

            def stored_freq(pl):
                L.get_compressed_freq(h, pl.out("f", np.full(snps, SENTINEL)))
                return pl.results()

            _sweep(stored_freq, {"f": ops.WIDE_OFFSETS}, devices=(False,))
    finally:
        L.free_compressed(ctypes.byref(h))


def test_results_and_frequencies_of_grm_and_ld_at_8_mod_16(mx):
    snps, indiv = 270, 135                                            # odd result dimension for the GRM: every second column starts at 8 mod 16 anyway
    prob = _problem(snps, indiv, 0.0)
    L = mx.lib.check_library_handle()

    def grm(pl):
        _ok(mx, L.mxa_grm(pl.inp("plink_t", prob["plink_t"]), snps, indiv, pl.out("G", np.full((indiv, indiv), SENTINEL)), 1, 1, pl.inp("f", prob["f"])))
        return pl.results()

    def ld(pl):
        _ok(mx, L.mxa_ld(pl.inp("plink", prob["plink"]), snps, indiv, pl.out("R", np.full((snps, snps), SENTINEL)), 1, pl.inp("f", prob["f"])))
        return pl.results()

    W = ops.WIDE_OFFSETS
    _sweep(grm, {"G": W, "f": W, "G+f": W})
    _sweep(ld, {"R": W, "f": W, "R+f": W})


# --------------------------------------------------------------------------------------------- 3. the windowed LD entries: doubles and integers
def test_outputs_windows_and_csr_of_the_windowed_ld_entries(mx):
    snps, indiv, w = 270, 526, 8                                      # ldb = w + 1 = 9: odd
    prob = _problem(snps, indiv, 0.0)
    X, f = prob["plink"], prob["f"]
    L = mx.lib.check_library_handle()
    last = ref.sweep_window(snps, 1)
    total = int(ref.rowptr_of(last)[-1])
    Xm = np.random.default_rng(4).standard_normal((3, snps + 1))      # ldx = snps + 1
    prio = np.random.default_rng(5).standard_normal(snps)
    W, I, B = ops.WIDE_OFFSETS, ops.INT_OFFSETS, ops.BYTE_OFFSETS

    def band(pl):
        _ok(mx, L.mxa_ld_band(pl.inp("plink", X), snps, indiv, w, pl.out("band", np.full((snps, w + 1), SENTINEL)), w + 1, 0, 1, pl.inp("f", f)))
        _ok(mx, L.mxa_ld_scores(pl.inp("plink", X), snps, indiv, w, pl.out("scores", np.full(snps, SENTINEL)), 1, 1, pl.inp("f", f)))
        return pl.results()

    def rows_scores(pl):
        _ok(mx, L.mxa_ld_window_rows(pl.inp("plink", X), snps, indiv, pl.inp("last", last), pl.out("rows", np.full(total, SENTINEL)), 1, 1, pl.inp("f", f)))
        _ok(mx, L.mxa_ld_window_scores(pl.inp("plink", X), snps, indiv, pl.inp("last", last), pl.out("scores", np.full(snps, SENTINEL)), 0, 1, pl.inp("f", f)))
        return pl.results()

    # the pairs, once, on aligned operands: the CSR the graph step takes
    tot = ctypes.c_long(-1)
    rp = np.zeros(snps + 1, np.int64)
    _ok(mx, L.mxa_ld_window_pairs(mx.lib.ptr(X), snps, indiv, mx.lib.ptr(last), MIN_R2, 0, mx.lib.ptr(rp), None, None, 0, ctypes.byref(tot), 1, mx.lib.ptr(f)))
    cap = tot.value
    assert cap > snps // 4
    col0, val0 = np.zeros(cap, np.int32), np.zeros(cap)
    _ok(mx, L.mxa_ld_window_pairs(mx.lib.ptr(X), snps, indiv, mx.lib.ptr(last), MIN_R2, 0, mx.lib.ptr(rp), mx.lib.ptr(col0), mx.lib.ptr(val0), cap, ctypes.byref(tot), 1,
                                  mx.lib.ptr(f)))

    def pairs(pl):
        t2 = ctypes.c_long(-1)
        _ok(mx, L.mxa_ld_window_pairs(pl.inp("plink", X), snps, indiv, pl.inp("last", last), MIN_R2, 1, pl.out("rowptr", np.full(snps + 1, -3, np.int64)),
                                      pl.out("col", np.full(cap, -3, np.int32)), pl.out("val", np.full(cap, SENTINEL)), cap, ctypes.byref(t2), 1, pl.inp("f", f)))
        assert t2.value == cap
        res = pl.results()
        assert np.array_equal(res[0], rp) and np.array_equal(res[1], col0) and np.array_equal(res[2], val0 * val0)
        return res

    def prune(pl):
        nk, rounds = ctypes.c_long(-1), ctypes.c_int(-1)
        _ok(mx, L.mxa_ld_window_prune(pl.inp("plink", X), snps, indiv, pl.inp("last", last), MIN_R2, pl.inp("priority", prio), pl.out("keep", np.full(snps, 9, np.uint8)),
                                      pl.out("owner", np.full(snps, -3, np.int32)), ctypes.byref(nk), ctypes.byref(rounds), 1, pl.inp("f", f)))
        res = pl.results()
        assert nk.value == int(res[0].sum()) and 0 < nk.value < snps
        return res

    def prune_csr(pl):
        nk, rounds = ctypes.c_long(-1), ctypes.c_int(-1)
        _ok(mx, L.mxa_ld_prune_csr(snps, pl.inp("rowptr", rp), pl.inp("col", col0), pl.inp("priority", prio), pl.out("keep", np.full(snps, 9, np.uint8)),
                                   pl.out("owner", np.full(snps, -3, np.int32)), ctypes.byref(nk), ctypes.byref(rounds)))
        res = pl.results()
        assert nk.value == int(res[0].sum())
        return res

    def apply(pl):
        for term in (0, 2):
            _ok(mx, L.mxa_ld_window_apply(pl.inp("plink", X), snps, indiv, pl.inp("last", last), term, pl.inp("X", Xm), snps + 1, 3,
                                          pl.out("Y", np.full((3, snps + 1), SENTINEL)), snps + 1, 1, pl.inp("f", f)))
        return pl.results()

    _sweep(band, {"band": W, "scores": W, "f": W})
    _sweep(rows_scores, {"rows": W, "scores": W, "last": I, "f": W})
    _sweep(pairs, {"rowptr": W, "col": (1,), "val": W, "rowptr+col+val": (1,), "last": I})
    _sweep(prune, {"keep": B, "owner": (1,), "keep+owner": (1,), "priority": W, "last": I})
    _sweep(prune_csr, {"rowptr": W, "col": (1, 2, 3), "priority": W, "keep": B, "owner": (1,), "keep+owner": (1,)})
    _sweep(apply, {"X": W, "Y": W, "X+Y": W, "last": I})


def test_the_ld_operator_object_at_offsets(mx):
    snps, indiv = 270, 526
    prob = _problem(snps, indiv, 0.0)
    X, f = prob["plink"], prob["f"]
    L = mx.lib.check_library_handle()
    last = ref.sweep_window(snps, 1)
    total = int(ref.rowptr_of(last)[-1])
    Xm = np.random.default_rng(4).standard_normal((3, snps + 1))
    W, I = ops.WIDE_OFFSETS, ops.INT_OFFSETS

    def use(pl, h):
        try:
            _ok(mx, L.mxa_ld_op_rows(h, pl.out("rows out", np.full(total, SENTINEL))))
            _ok(mx, L.mxa_ld_op_apply(h, 0.5, pl.inp("X", Xm), snps + 1, 3, pl.out("Y", np.full((3, snps + 1), SENTINEL)), snps + 1))
            _ok(mx, L.mxa_ld_op_solve(h, 2.0, pl.inp("B", Xm), snps + 1, 3, pl.out("Xs", np.full((3, snps + 1), SENTINEL)), snps + 1, 1e-10, 500,
                                      pl.out("iters", np.full(3, -3, np.int32), device=False), pl.out("relres", np.full(3, SENTINEL), device=False),
                                      pl.out("status", np.full(3, -3, np.int32), device=False)))
        finally:
            L.mxa_ld_op_free(ctypes.byref(h))
        res = pl.results()
        assert np.all(res[5] == 0), "converged"
        return res

    def created(pl):
        h = ctypes.c_void_p(None)
        _ok(mx, L.mxa_ld_op_create(pl.inp("plink", X), snps, indiv, pl.inp("last", last), 1, 1, pl.inp("f", f), ctypes.byref(h)))
        return use(pl, h)

    rows0 = created(Place())[0]

    def from_rows(pl):
        h = ctypes.c_void_p(None)
        _ok(mx, L.mxa_ld_op_from_rows(snps, pl.inp("last", last, device=False), pl.inp("rows", rows0), ctypes.byref(h)))
        return use(pl, h)

    _sweep(created, {"last": I, "f": W, "rows out": W, "X": W, "Y": W, "X+Y": W, "B": W, "Xs": W, "B+Xs": W, "iters": I, "relres": W, "status": I,
                     "plink": ops.BYTE_OFFSETS})
    _sweep(from_rows, {"rows": W, "last": I})
    _same(from_rows(Place()), created(Place()), "from_rows on the exported rows")
