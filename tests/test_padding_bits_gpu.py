"""The padding fields of a packed row's last byte (the fields at and beyond the row's length) with something other than 00 in them: a memory-mapped .bed
written by another tool, a torch slice, a buffer that is reused.  include/miraculix_amd.h states for every entry group what they mean; this module holds the
library to it.  The four patterns of tests/_operands.py (01, 10, 11 everywhere, and a seeded pick per row) against the call on clean padding IN THE SAME PROCESS:

  IGNORED, the same bits as the clean call (uint64 views, NaNs included): plink2compressed in every call shape, the sharded, incremental and .bed staging,
    get_compressed_freq, dgemm_compressed 'N' / 'T' (n = 1, 2, 3, 8, 33: lookup kernel, guarded int8 route, fp64 MFMA, column chunks and peel; centred and not;
    one-copy and two-copy objects; MIRACULIX_NUM_GPUS=3), mxa_gram_matvec, dgemm_plink, sparse_times_plink, mxa_transpose_2bit (whose output has zero
    padding), mxa_allele_freq, every _pairwise entry, and the plain GRM / LD entries (mxa_grm, mxa_ld, mxa_ld_band, mxa_ld_scores, mxa_ld_window_*,
    mxa_ld_op_create; fused and MXA_XPROD_FUSED_POST=0).
  AS STORED, the reference's behaviour (it multiplies whole bytes): snp_multiply_gpu and mxa_snp_multiply_panel equal Oracle.crossprod_i32 ON THE DIRTY BYTES
    exactly -- and differ from the clean result, which proves that the padding takes part.

The clean call itself is checked once against the reference its own tests use, at their tolerance: the oracle (1e-11 of the largest entry for the fp64
products, 1e-13 for the sparse product, exact for the integer entries), tests/_ld_ref.py (element bound of the LD map, 8 units on the pairwise route, the scores'
summation bound), tests/_ld_apply_ref.py ((m + 2) u sum |t x|), tests/_ld_prune_ref.py (the sequential walk)."""
import ctypes

import numpy as np
import pytest

import _ld_apply_ref as ar
import _ld_prune_ref as pr
import _ld_ref as ref
import _operands as ops
from _util import Oracle, make_B, make_problem, pack_plink, random_csr, synth_genotypes

pytestmark = pytest.mark.gpu

U = ref.U
SENTINEL = -12345.678
NS = (1, 2, 3, 8, 33)
MIN_R2 = 0.004                           # a few per cent of the pairs at 1031 individuals, most of them at 70


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@pytest.fixture(autouse=True)
def _default_environment(monkeypatch):
    for name in ("MXA_XPROD_ENGINE", "MXA_XPROD_FUSED_POST", "MXA_SINGLE_ORIENTATION", "MIRACULIX_NUM_GPUS", "MXA_LD_PAIRWISE_SCRATCH_MB", "MXA_LD_PAIRWISE_DENSE",
                 "MXA_XPROD_NO_PIPELINE", "MXA_XPROD_HOST_RING"):
        monkeypatch.delenv(name, raising=False)
    yield
    _HELD.clear()


# --------------------------------------------------------------------------------------------------------------------------------------- tools
_PROBLEMS = {}


def _problem(snps, indiv, missing_frac=0.05):
    key = (snps, indiv, missing_frac)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = make_problem(snps, indiv, 1, seed=snps + indiv, missing_frac=missing_frac)
    return _PROBLEMS[key]


def _patterns(P, k):
    """(code, dirty copy) for the four patterns; every one differs from P in every row's last byte"""
    assert ops.padding_fields(k) > 0, k
    out = []
    for code in ops.CODES:
        D = ops.dirty(P, k, code)
        assert np.all(D[:, -1] != P[:, -1]) and np.array_equal(D[:, :-1], P[:, :-1])
        out.append((code, D))
    return out


_HELD = []                                # device copies stay alive until the test ends: p(_dev(a)) inside a call's argument list must not dangle


def _dev(a):
    import torch
    if a is None:
        return None
    _HELD.append(torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0)))
    return _HELD[-1]


def _host(a):
    if hasattr(a, "detach"):
        import torch
        torch.cuda.synchronize()
        return a.detach().cpu().numpy()
    return a


def _same(got, want, what):
    """every array of `got` holds the bits of its twin in `want`"""
    assert len(got) == len(want), what
    for q, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(_host(g)), np.ascontiguousarray(_host(w))
        assert g.shape == w.shape and g.dtype == w.dtype, (what, q)
        assert np.array_equal(ops.bits(g), ops.bits(w)), (what, q, int((ops.bits(g) != ops.bits(w)).sum()))


def _close(got, want, rtol, what):
    scale = max(float(np.abs(want).max()), 1e-300)
    err = float(np.abs(got - want).max()) / scale
    assert err <= rtol, (what, err)


# ------------------------------------------------------------------------------------------------------------------- 1. the compressed objects
HOWS = ("two pointers", "one pointer", "same pointer", "device source", "device both")


def _create(mx, how, P, Pt, snps, indiv, f, max_n=33):
    """plink2compressed in the call shape `how` through the raw entry; returns the handle"""
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    h = ctypes.c_void_p(None)
    keep = []
    if how == "two pointers":
        a, b = p(P), p(Pt)
    elif how == "one pointer":
        a, b = p(P), None
    elif how == "same pointer":
        a, b = p(P), p(P)
    elif how == "device source":
        keep = [_dev(P)]
        a, b = p(keep[0]), None
    else:
        keep = [_dev(P), _dev(Pt)]
        a, b = p(keep[0]), p(keep[1])
    L.plink2compressed(a, b, snps, indiv, p(f), max_n, ctypes.byref(h))
    assert h.value, mx.lib.last_error()
    return h


def _free(mx, h):
    mx.lib.check_library_handle().free_compressed(ctypes.byref(h))


def _operands_B(snps, indiv):
    """{(trans, n): B as (n, ldb) rows = columns, ldb = k + 3 with poisoned padding}"""
    return {(t, n): make_B(indiv if t else snps, n, seed=11 + 2 * n + t, ldb=(indiv if t else snps) + 3) for t in (0, 1) for n in NS}


def _products(mx, h, snps, indiv, Bs, rows_of=None):
    """[C(trans, n) for every operand, the stored frequencies, mxa_gram_matvec at n = 3]: raw calls, ldc = m + 2 with sentinels behind every column.
    rows_of = (b, e): the object is the SNP shard [b, e)"""
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    b, e = rows_of or (0, snps)
    out = []
    for (t, n), B in sorted(Bs.items()):
        m = (e - b) if t else indiv
        ldb, ldc = B.shape[1], m + 2
        Bv = B if t else np.ascontiguousarray(B[:, b:])              # 'N' on a shard: rows [b, e) of B
        C = np.full((n + 1, ldc), SENTINEL)
        L.dgemm_compressed(b"T" if t else b"N", h, n, p(Bv), Bv.shape[1] if not t else ldb, p(C), ldc)
        assert L.mxa_last_error() == 0, mx.lib.last_error()
        assert np.all(C[n] == SENTINEL) and np.all(C[:n, m:] == 0.0), "dgemm_compressed zero-fills rows m .. ldc - 1 and writes nothing behind column n - 1"
        out.append(C[:n, :m].copy())
    f = np.full(snps + 1, SENTINEL)
    L.get_compressed_freq(h, p(f))
    out.append(f[: e - b + 1].copy() if rows_of else f.copy())
    V = make_B(indiv, 3, seed=5)
    G = np.full((4, indiv), SENTINEL)
    assert L.mxa_gram_matvec(h, 3, p(V), indiv, p(G), indiv) == 0, mx.lib.last_error()
    assert np.all(G[3] == SENTINEL)
    # the fused step is 'T' then 'N' with the intermediate kept on the device: the same bits as the two calls (tests/test_cg_gpu.py)
    W, G2 = np.zeros((3, e - b)), np.zeros((3, indiv))
    L.dgemm_compressed(b"T", h, 3, p(V), indiv, p(W), e - b)
    L.dgemm_compressed(b"N", h, 3, p(W), e - b, p(G2), indiv)
    assert L.mxa_last_error() == 0 and np.array_equal(ops.bits(G[:3]), ops.bits(G2))
    out.append(G[:3].copy())
    return out


def _check_products(oracle, prob, Bs, res, centered, what):
    """the clean object's products against the dense oracle at the suite's 1e-11, the frequencies as given, the fused step as its two products"""
    snps, indiv = prob["snps"], prob["indiv"]
    for ((t, n), B), C in zip(sorted(Bs.items()), res):
        want = oracle.dgemm_dense(t, prob, B, centered)[:, : (snps if t else indiv)]
        _close(C, want, 1e-11, (what, t, n))
    f = res[len(Bs)]
    assert np.array_equal(f[:snps], prob["f"]) and f[snps] == SENTINEL, what


@pytest.mark.parametrize("single", ["0", "1"])
@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("snps,indiv", ops.PADDING_OBJECT_SHAPES)
def test_compressed_objects_ignore_the_padding(mx, oracle, monkeypatch, snps, indiv, how, single):
    monkeypatch.setenv("MXA_SINGLE_ORIENTATION", single)
    prob = _problem(snps, indiv)
    P, Pt, f = prob["plink"], prob["plink_t"], prob["f"]
    Bs = _operands_B(snps, indiv)
    L = mx.lib.check_library_handle()
    for centered in (True, False):
        mx.dgemm_compressed.set_options(use_gpu=True, not_center=not centered, verbose=0)
        h = _create(mx, how, P, Pt, snps, indiv, f)
        try:
            assert L.mxa_single_orientation(h) == int(single)
            clean = _products(mx, h, snps, indiv, Bs)
        finally:
            _free(mx, h)
        _check_products(oracle, prob, Bs, clean, int(centered), (how, single, centered))
        for (code, D), (_, Dt) in zip(_patterns(P, indiv), _patterns(Pt, snps)):
            h = _create(mx, how, D, Dt, snps, indiv, f)
            try:
                _same(_products(mx, h, snps, indiv, Bs), clean, (how, single, centered, code))
            finally:
                _free(mx, h)
    mx.dgemm_compressed.set_options(use_gpu=True, not_center=False, verbose=0)


@pytest.mark.parametrize("how", ["two pointers", "one pointer"])
@pytest.mark.parametrize("snps,indiv", ops.PADDING_OBJECT_SHAPES)
def test_three_shards_behind_one_handle_ignore_the_padding(mx, oracle, monkeypatch, snps, indiv, how):
    prob = _problem(snps, indiv)
    P, Pt, f = prob["plink"], prob["plink_t"], prob["f"]
    Bs = _operands_B(snps, indiv)
    L = mx.lib.check_library_handle()
    mx.dgemm_compressed.set_options(use_gpu=True, not_center=False, verbose=0)

    def run(A, At):
        monkeypatch.setenv("MIRACULIX_NUM_GPUS", "3")
        h = _create(mx, how, A, At, snps, indiv, f)
        monkeypatch.delenv("MIRACULIX_NUM_GPUS")
        try:
            assert L.mxa_num_shards(h) == 3
            return _products(mx, h, snps, indiv, Bs)
        finally:
            _free(mx, h)

    clean = run(P, Pt)
    _check_products(oracle, prob, Bs, clean, 1, how)
    for (code, D), (_, Dt) in zip(_patterns(P, indiv), _patterns(Pt, snps)):
        _same(run(D, Dt), clean, (how, code))


@pytest.mark.parametrize("snps,indiv", ops.PADDING_OBJECT_SHAPES)
def test_sharded_incremental_and_bed_staging_ignore_the_padding(mx, oracle, tmp_path, snps, indiv):
    prob = _problem(snps, indiv)
    P, Pt, f = prob["plink"], prob["plink_t"], prob["f"]
    Bs = _operands_B(snps, indiv)
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    dg = mx.dgemm_compressed
    dg.set_options(use_gpu=True, not_center=False, verbose=0)
    cut = 32 if snps < 128 else 128                                   # shard boundaries are multiples of 4
    f_counted = oracle.allele_freq(P, snps, indiv)

    def shards(A, At):
        out = []
        for b, e in ((0, cut), (cut, snps)):
            for with_t in (True, False):
                h = ctypes.c_void_p(None)
                L.mxa_plink2compressed_shard(p(A), p(At) if with_t else None, snps, indiv, b, e, p(f), 33, ctypes.byref(h))
                assert h.value, mx.lib.last_error()
                try:
                    out += _products(mx, h, snps, indiv, Bs, rows_of=(b, e))[: len(Bs)]
                finally:
                    _free(mx, h)
        return out

    def incremental(A, device):
        h = dg.init_compressed_begin(snps, indiv, 33)
        try:
            for b, e in ((cut, snps), (0, cut)):                      # any order; the frequencies are counted on the device
                rows = np.ascontiguousarray(A[b:e])
                dg.append_rows(h, _dev(rows) if device else rows, b)
            fq = dg.init_compressed_end(h, snps)
            return _products(mx, h, snps, indiv, Bs)[: len(Bs)] + [fq]
        finally:
            _free(mx, h)

    def bed(A, name):
        base = str(tmp_path / name)
        mx.read_plink.write_bed(base + ".bed", A)
        with open(base + ".bim", "w") as fh:
            fh.write("".join(f"1 snp{i} 0 {i} A B\n" for i in range(snps)))
        with open(base + ".fam", "w") as fh:
            fh.write("".join(f"f{i} i{i} 0 0 0 -9\n" for i in range(indiv)))
        out = []
        h, fq, s2, i2 = dg.init_compressed_from_bed(base + ".bed", 33)
        try:
            assert (s2, i2) == (snps, indiv)
            out += _products(mx, h, snps, indiv, Bs)[: len(Bs)] + [fq]
        finally:
            _free(mx, h)
        h, fq = dg.init_compressed_from_bed_range(base + ".bed", cut, snps, 33)
        try:
            out += _products(mx, h, snps, indiv, Bs, rows_of=(cut, snps))[: len(Bs)] + [fq]
        finally:
            _free(mx, h)
        return out

    keys = sorted(Bs)
    clean_sh = shards(P, Pt)
    nB = len(Bs)
    for q, (t, n) in enumerate(keys):                                 # the two shards together are the whole product ('T': row blocks; 'N': partial sums)
        want = oracle.dgemm_dense(t, prob, Bs[(t, n)], 1)[:, : (snps if t else indiv)]
        for v in (0, 1):                                              # with and without plink_transposed
            lo, hi = clean_sh[(0 + v) * nB + q], clean_sh[(2 + v) * nB + q]
            _close(np.concatenate([lo, hi], axis=1) if t else lo + hi, want, 1e-11, ("shards", t, n, v))
    clean_inc = [incremental(P, d) for d in (False, True)]
    clean_bed = bed(P, "clean")
    prob_counted = dict(prob, f=f_counted)                            # these objects multiply with the frequencies counted on the device
    for res in clean_inc + [clean_bed[: nB + 1]]:
        assert np.array_equal(res[nB], f_counted)
        for q, (t, n) in enumerate(keys):
            _close(res[q], oracle.dgemm_dense(t, prob_counted, Bs[(t, n)], 1)[:, : (snps if t else indiv)], 1e-11, ("staged", t, n))
    assert np.array_equal(clean_bed[2 * nB + 1], f_counted[cut:])
    for (code, D), (_, Dt) in zip(_patterns(P, indiv), _patterns(Pt, snps)):
        _same(shards(D, Dt), clean_sh, ("shards", code))
        for d in (False, True):
            _same(incremental(D, d), clean_inc[d], ("incremental", d, code))
        _same(bed(D, f"dirty{code}"), clean_bed, (".bed", code))


# ---------------------------------------------------------------------------------------------------------- 2. entries without an object
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("snps,indiv", ops.PADDING_OBJECT_SHAPES)
def test_transpose_frequencies_dgemm_plink_and_sparse_ignore_the_padding(mx, oracle, snps, indiv, device):
    prob = _problem(snps, indiv)
    P, Pt, f = prob["plink"], prob["plink_t"], prob["f"]
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    to = _dev if device else (lambda a: a)
    mx.dgemm_compressed.set_options(use_gpu=True, not_center=False, verbose=0)
    csr = {tc: random_csr(9, indiv if tc else snps, 12, seed=3 + tc) for tc in (0, 1)}
    Bn, Bt = make_B(snps, 3, seed=7), make_B(indiv, 3, seed=8)

    def run(A, At):
        out = []
        # the transposes, both ways, into buffers with sentinel bytes behind them
        for src, rows, cols in ((A, snps, indiv), (At, indiv, snps)):
            nout = cols * ((rows + 3) // 4)
            T = to(np.full(nout + 8, 0xA5, np.uint8))
            assert L.mxa_transpose_2bit(p(to(src)), rows, cols, p(T)) == 0, mx.lib.last_error()
            T = _host(T)
            assert np.all(T[nout:] == 0xA5)
            out.append(T[:nout].reshape(cols, -1).copy())
        for src, rows, cols in ((A, snps, indiv), (At, indiv, snps)):
            fq = to(np.full(rows + 1, SENTINEL))
            assert L.mxa_allele_freq(p(to(src)), rows, cols, p(fq)) == 0, mx.lib.last_error()
            fq = _host(fq)
            assert fq[rows] == SENTINEL
            out.append(fq[:rows].copy())
        for t in (0, 1):
            for freq in (f, None):
                m, B = (snps, Bt) if t else (indiv, Bn)
                C = to(np.full((4, m + 1), SENTINEL))
                L.dgemm_plink(b"T" if t else b"N", p(to(A)) if t else None, None if t else p(to(At)), snps, indiv, p(freq), 3, p(to(B)), B.shape[1], p(C), m + 1)
                assert L.mxa_last_error() == 0, mx.lib.last_error()
                C = _host(C)
                assert np.all(C[3] == SENTINEL)
                out.append(C[:3, :m].copy())
        for tc in (0, 1):
            ia, ja, a = csr[tc]
            entries = snps if tc else indiv
            C = to(np.full((entries + 1, 11), SENTINEL))              # column-major 11 x entries (ldc = 11 >= nIdx = 9) and one guard column
            L.sparse_times_plink(b"N", b"T" if tc else b"N", None if tc else p(to(A)), p(to(At)) if tc else None, snps, indiv, 9, p(to(ia)), p(to(ja)), p(to(a)), p(C), 11)
            assert L.mxa_last_error() == 0, mx.lib.last_error()
            C = _host(C)
            assert np.all(C[entries] == SENTINEL) and np.all(C[:entries, 9:] == 0.0)
            out.append(C[:entries, :9].copy())
        return out

    clean = run(P, Pt)
    assert np.array_equal(clean[0], Pt) and np.array_equal(clean[1], P)                  # pack_plink's own rows: zero padding
    assert np.array_equal(clean[0], oracle.transpose_2bit(P, snps, indiv)) and np.array_equal(clean[1], oracle.transpose_2bit(Pt, indiv, snps))
    assert np.array_equal(clean[2], oracle.allele_freq(P, snps, indiv)) and np.array_equal(clean[3], oracle.allele_freq(Pt, indiv, snps))
    q = 4
    for t in (0, 1):
        for centered in (1, 0):
            want = oracle.dgemm_dense(t, prob, Bt if t else Bn, centered)[:, : (snps if t else indiv)]
            _close(clean[q], want, 1e-11, ("dgemm_plink", t, centered))
            q += 1
    for tc in (0, 1):
        ia, ja, a = csr[tc]
        rows, entries = (indiv, snps) if tc else (snps, indiv)
        want = oracle.sparse_times_plink(Pt if tc else P, rows, entries, ia, ja, a)
        assert np.abs(clean[q] - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), ("sparse_times_plink", tc)
        q += 1
    for (code, D), (_, Dt) in zip(_patterns(P, indiv), _patterns(Pt, snps)):
        got = run(D, Dt)
        for T, k in ((got[0], snps), (got[1], indiv)):                # the output's own padding is zero, whatever the input's was
            assert np.all(T[:, -1] >> (2 * (k % 4)) == 0), code
        _same(got, clean, code)


# ------------------------------------------------------------------------------------------------------------------- 3. the windowed LD entries
def _windows(snps):
    return [(w, ref.fixed_last(snps, w)) for w in (0, 7, snps - 1)]


def _ld_entries(mx, X, snps, indiv, f, pairwise, device=False, full=True, windows=True):
    """every LD entry of one route on the packed matrix X through the raw C entries, outputs behind sentinels: {name: array}.  f: the plain route's
    frequencies (pairwise: None)"""
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    to = _dev if device else (lambda a: a)
    sfx = "_pairwise" if pairwise else ""
    tail = [] if pairwise else [1, p(to(f))]
    Xd = to(X)
    out = {}
    if full and not pairwise:
        R = to(np.full(snps * snps + 3, SENTINEL))
        assert L.mxa_ld(p(Xd), snps, indiv, p(R), 1, p(to(f))) == 0, mx.lib.last_error()
        R = _host(R)
        assert np.all(R[snps * snps:] == SENTINEL)
        out["ld"] = R[: snps * snps].reshape(snps, snps).copy()
    if not windows:
        return out
    Xm = np.random.default_rng([snps, 3]).standard_normal((3, snps))     # three columns of X, column-major
    prio = np.random.default_rng([snps, 4]).standard_normal(snps)
    for w, last in _windows(snps):
        total = int(ref.rowptr_of(last)[-1])
        lastd = to(last)
        for kind in (0, 1):
            ldb = w + 3
            B = to(np.full((snps + 1, ldb), SENTINEL))
            assert getattr(L, "mxa_ld_band" + sfx)(p(Xd), snps, indiv, w, p(B), ldb, kind, *tail) == 0, mx.lib.last_error()
            B = _host(B)
            assert np.all(B[snps] == SENTINEL) and np.all(B[:, w + 1:] == SENTINEL)
            out["band", w, kind] = B[:snps, : w + 1].copy()
            rows = to(np.full(total + 5, SENTINEL))
            assert getattr(L, "mxa_ld_window_rows" + sfx)(p(Xd), snps, indiv, p(lastd), p(rows), kind, *tail) == 0, mx.lib.last_error()
            rows = _host(rows)
            assert np.all(rows[total:] == SENTINEL)
            out["rows", w, kind] = rows[:total].copy()
            h = ctypes.c_void_p(None)
            if pairwise:
                rc = L.mxa_ld_op_create_pairwise(p(Xd), snps, indiv, p(lastd), kind, ctypes.byref(h))
            else:
                rc = L.mxa_ld_op_create(p(Xd), snps, indiv, p(lastd), kind, 1, p(to(f)), ctypes.byref(h))
            assert rc == 0 and h.value, mx.lib.last_error()
            try:
                back = np.full(total + 5, SENTINEL)
                assert L.mxa_ld_op_rows(h, p(back)) == 0 and np.all(back[total:] == SENTINEL)
                Y = np.full((4, snps + 2), SENTINEL)
                assert L.mxa_ld_op_apply(h, 0.5, p(Xm), snps, 3, p(Y), snps + 2) == 0, mx.lib.last_error()
                assert np.all(Y[3] == SENTINEL) and np.all(Y[:3, snps:] == SENTINEL)
                out["op rows", w, kind], out["op apply", w, kind] = back[:total].copy(), Y[:3, :snps].copy()
            finally:
                L.mxa_ld_op_free(ctypes.byref(h))
        for adjust in (0, 1):
            for name, arg in (("mxa_ld_scores", w), ("mxa_ld_window_scores", p(lastd))):
                S = to(np.full(snps + 2, SENTINEL))
                assert getattr(L, name + sfx)(p(Xd), snps, indiv, arg, p(S), adjust, *tail) == 0, mx.lib.last_error()
                S = _host(S)
                assert np.all(S[snps:] == SENTINEL)
                out[name, w, adjust] = S[:snps].copy()
        # pairs: count, then fill into exactly sized arrays with a guard entry
        rowptr = to(np.full(snps + 2, -7, np.int64))
        tot = ctypes.c_long(-1)
        assert getattr(L, "mxa_ld_window_pairs" + sfx)(p(Xd), snps, indiv, p(lastd), MIN_R2, 0, p(rowptr), None, None, 0, ctypes.byref(tot), *tail) == 0, mx.lib.last_error()
        cap = tot.value
        col, val = to(np.full(cap + 1, -7, np.int32)), to(np.full(cap + 1, SENTINEL))
        assert getattr(L, "mxa_ld_window_pairs" + sfx)(p(Xd), snps, indiv, p(lastd), MIN_R2, 0, p(rowptr), p(col), p(val), cap, ctypes.byref(tot), *tail) == 0
        rowptr, col, val = _host(rowptr), _host(col), _host(val)
        assert tot.value == cap == rowptr[snps] and rowptr[snps + 1] == -7 and col[cap] == -7 and val[cap] == SENTINEL
        out["pairs rowptr", w], out["pairs col", w], out["pairs val", w] = rowptr[: snps + 1].copy(), col[:cap].copy(), val[:cap].copy()
        keep, owner = to(np.full(snps + 1, 9, np.uint8)), to(np.full(snps + 1, -7, np.int32))
        nk, rounds = ctypes.c_long(-1), ctypes.c_int(-1)
        assert getattr(L, "mxa_ld_window_prune" + sfx)(p(Xd), snps, indiv, p(lastd), MIN_R2, p(to(prio)), p(keep), p(owner), ctypes.byref(nk), ctypes.byref(rounds), *tail) == 0
        keep, owner = _host(keep), _host(owner)
        assert keep[snps] == 9 and owner[snps] == -7 and nk.value == int(keep[:snps].sum())
        out["prune keep", w], out["prune owner", w] = keep[:snps].copy(), owner[:snps].copy()
        for term in (0, 1, 2):
            Y = to(np.full((4, snps + 2), SENTINEL))
            assert getattr(L, "mxa_ld_window_apply" + sfx)(p(Xd), snps, indiv, p(lastd), term, p(to(Xm)), snps, 3, p(Y), snps + 2, *tail) == 0, mx.lib.last_error()
            Y = _host(Y)
            assert np.all(Y[3] == SENTINEL) and np.all(Y[:3, snps:] == SENTINEL)
            out["apply", w, term] = Y[:3, :snps].copy()
    out["_X"], out["_prio"] = Xm, prio
    return out


def _check_ld_entries(res, snps, indiv, r, b, N, pairwise):
    """the clean results of _ld_entries against the references of the entries' own tests.  r: the long-double reference (snps x snps), b: the allowed
    |r^ - r| per element, N: the pairwise route's N_ij (plain: None)"""
    ii_all = np.arange(snps)
    Xm, prio = res["_X"], res["_prio"]
    for w, last in _windows(snps):
        ii, jj = ref.pairs(last)
        rows = res["rows", w, 0]
        nan = np.isnan(r[ii, jj].astype(np.float64))
        assert np.array_equal(np.isnan(rows), nan), w
        assert ref.worst_ratio(rows[~nan], r[ii, jj][~nan], b[ii, jj][~nan]) <= 1.0, w
        assert np.array_equal(ops.bits(res["rows", w, 1]), ops.bits(rows * rows)), w
        inband = (ii_all[:, None] + np.arange(w + 1)[None, :]) < snps
        for kind in (0, 1):
            band = res["band", w, kind]
            assert np.array_equal(ops.bits(band[inband]), ops.bits(res["rows", w, kind])), (w, kind)      # the band's row i is the ragged row i
            assert np.all(band[~inband] == 0.0)
            assert np.array_equal(ops.bits(res["op rows", w, kind]), ops.bits(res["rows", w, kind])), (w, kind)
            T = ar.dense(res["rows", w, kind], last)
            want, mag, m = ar.apply_ref(T, last, Xm.T)
            full = want.astype(ref.LD) + ref.LD(0.5) * Xm.T.astype(ref.LD)
            bound = (m[:, None] + 3.0) * U * (mag + np.abs(0.5 * Xm.T) * (1.0 - 2.0 ** -40))
            ok = np.isfinite(want)
            got = res["op apply", w, kind].T
            assert np.array_equal(np.isfinite(got), ok) and np.all(np.abs(got.astype(ref.LD) - full).astype(np.float64)[ok] <= bound[ok]), (w, kind)
        if "ld" in res:
            assert np.array_equal(ops.bits(res["ld"][ii, jj]), ops.bits(rows)), w
        R0 = ar.dense(rows, last)
        for term in (0, 1, 2):
            T = ar.terms_pw(R0, N, term) if pairwise else ar.terms(R0, indiv, term)
            want, mag, m = ar.apply_ref(T, last, Xm.T)
            ok = np.isfinite(want)
            got = res["apply", w, term].T
            assert np.array_equal(np.isfinite(got), ok), (w, term)
            assert np.all(np.abs(got - want)[ok] <= ((m[:, None] + 2.0) * U * mag)[ok]), (w, term)
        for adjust in (0, 1):
            g = 0.0 if not adjust else (1.0 / (N - 2.0) if pairwise else 1.0 / (indiv - 2.0))
            want, tol = ref.scores_ref(r, b, g, last)
            ok = np.isfinite(want)
            for name in ("mxa_ld_scores", "mxa_ld_window_scores"):
                S = res[name, w, adjust]
                assert np.array_equal(np.isfinite(S), ok) and np.all(np.abs(S - want)[ok] <= tol[ok]), (name, w, adjust)
            assert np.array_equal(ops.bits(res["mxa_ld_scores", w, adjust]), ops.bits(res["mxa_ld_window_scores", w, adjust])), (w, adjust)
        # the pairs are the rows' entries above the cutoff; the pruning is the sequential walk on them
        with np.errstate(invalid="ignore"):
            hit = (jj > ii) & (rows * rows >= MIN_R2)
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(ii[hit], minlength=snps))]).astype(np.int64)
        assert np.array_equal(res["pairs rowptr", w], rowptr) and np.array_equal(res["pairs col", w], jj[hit].astype(np.int32)), w
        assert np.array_equal(ops.bits(res["pairs val", w]), ops.bits(rows[hit])), w
        keep, owner = pr.ref_greedy(snps, rowptr, jj[hit], prio)
        assert np.array_equal(res["prune keep", w].astype(bool), keep) and np.array_equal(res["prune owner", w], owner), w


def _same_entries(got, want, what):
    assert got.keys() == want.keys()
    for key in want:
        _same([got[key]], [want[key]], (what, key))


@pytest.mark.parametrize("snps,indiv", ops.PADDING_OBJECT_SHAPES)
def test_pairwise_ld_entries_ignore_the_padding(mx, monkeypatch, snps, indiv):
    X = _problem(snps, indiv)["plink"]
    assert (ref.codes(X, indiv) == 1).any()
    clean = _ld_entries(mx, X, snps, indiv, None, True)
    case = ref.pairwise_restate(X, indiv)
    _check_ld_entries(clean, snps, indiv, case["r"], ref.pairwise_bound(case["r"]), case["N"].astype(np.float64), True)
    for code, D in _patterns(X, indiv):
        _same_entries(_ld_entries(mx, D, snps, indiv, None, True, device=code == "random"), clean, ("pairwise", code))
    monkeypatch.setenv("MXA_XPROD_ENGINE", "i8")
    _same_entries(_ld_entries(mx, ops.dirty(X, indiv, "random"), snps, indiv, None, True), clean, ("pairwise", "int8 engine"))


@pytest.mark.parametrize("snps,indiv", ops.PADDING_LD_SHAPES)
def test_plain_ld_entries_ignore_the_padding(mx, monkeypatch, snps, indiv):
    """mxa_ld, mxa_ld_band, mxa_ld_scores, mxa_ld_window_rows / _scores / _pairs / _prune / _apply, mxa_ld_op_create: the padding fields are no individuals
    (as in `indiv` and f of their own formula).  Before the staging kernel masked them, a padding 01 turned the row's last byte into four 3s and a padding
    10 / 11 added a phantom individual to sum z z': every entry of this test differed from the clean call."""
    prob = _problem(snps, indiv, 0.0)
    X, f = prob["plink"], prob["f"]
    clean = _ld_entries(mx, X, snps, indiv, f, False)
    case = ref.plain_case(X, indiv, f)
    assert np.isfinite(case["b"]).all()
    _check_ld_entries(clean, snps, indiv, case["r"], case["b"], None, False)
    for code, D in _patterns(X, indiv):
        _same_entries(_ld_entries(mx, D, snps, indiv, f, False, device=code == "random"), clean, ("plain", code))
    D = ops.dirty(X, indiv, "random")
    monkeypatch.setenv("MXA_XPROD_FUSED_POST", "0")
    _same([_ld_entries(mx, D, snps, indiv, f, False, windows=False)["ld"]], [clean["ld"]], "mxa_ld, three passes")
    monkeypatch.delenv("MXA_XPROD_FUSED_POST")
    monkeypatch.setenv("MXA_XPROD_ENGINE", "i8")
    _same_entries(_ld_entries(mx, D, snps, indiv, f, False), clean, ("plain", "int8 engine"))


def _grm_ref(Z, f, do_scale):
    """crossproduct.jl:94-107 (tests/test_grm_ld_fused_gpu.py)"""
    M = Z @ Z.T
    n = M.shape[0]
    cs = M.sum(axis=0)
    M = M - np.outer(cs, np.ones(n)) / n - np.outer(np.ones(n), cs) / n + cs.sum() / n ** 2
    return M / (2 * np.sum(f * (1 - f))) if do_scale else M


@pytest.mark.parametrize("snps,indiv", ops.PADDING_GRM_SHAPES)
def test_grm_and_ld_ignore_the_padding_fused_and_in_three_passes(mx, monkeypatch, snps, indiv):
    prob = _problem(snps, indiv, 0.0)
    Pt, f = prob["plink_t"], prob["f"]
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    raw = np.random.default_rng([snps, indiv]).integers(0, 256, Pt.shape, dtype=np.uint8)
    raw[:, -1] &= np.uint8((1 << (2 * (snps % 4))) - 1)                # raw 2-bit fields (is_plink_format = 0) with clean padding

    def run(A, is_plink, device, engine=None, fused=None):
        to = _dev if device else (lambda a: a)
        if engine:
            monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
        if fused is not None:
            monkeypatch.setenv("MXA_XPROD_FUSED_POST", fused)
        out = []
        for do_scale in (1, 0):
            G = to(np.full(indiv * indiv + 3, SENTINEL))
            assert L.mxa_grm(p(to(A)), snps, indiv, p(G), is_plink, do_scale, p(to(f))) == 0, mx.lib.last_error()
            G = _host(G)
            assert np.all(G[indiv * indiv:] == SENTINEL)
            out.append(G[: indiv * indiv].reshape(indiv, indiv).copy())
        monkeypatch.delenv("MXA_XPROD_ENGINE", raising=False)
        monkeypatch.delenv("MXA_XPROD_FUSED_POST", raising=False)
        return out

    Z = prob["Z"].astype(np.float64)
    for is_plink, A in ((1, Pt), (0, raw)):
        clean = run(A, is_plink, False)
        if is_plink:
            for do_scale, G in zip((1, 0), clean):
                want = _grm_ref(Z, f, do_scale)
                assert np.abs(G - want).max() <= 1e-12 * np.abs(want).max()
        _same(run(A, is_plink, False, fused="0"), clean, "clean, three passes")
        for code, D in _patterns(A, snps):
            _same(run(D, is_plink, False), clean, (is_plink, code))
            _same(run(D, is_plink, False, fused="0"), clean, (is_plink, code, "three passes"))
        D = ops.dirty(A, snps, "random")
        _same(run(D, is_plink, True), clean, (is_plink, "device"))
        _same(run(D, is_plink, False, engine="i8"), clean, (is_plink, "int8 engine"))


# --------------------------------------------------------------------------------------------------------- 4. the crossproduct: as stored
@pytest.mark.parametrize("engine", ["f4", "i8"])
@pytest.mark.parametrize("is_plink", [False, True])
@pytest.mark.parametrize("k,rows", ops.PADDING_XPROD_SHAPES)
def test_crossproduct_multiplies_the_padding_as_stored(mx, oracle, monkeypatch, k, rows, is_plink, engine):
    """snp_multiply_gpu and mxa_snp_multiply_panel: the reference multiplies whole bytes (and under the PLINK table a padding 01 turns its byte into four 3s),
    so the result on dirty padding is the oracle's on the same bytes -- and not the clean result"""
    monkeypatch.setenv("MXA_XPROD_ENGINE", engine)
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    if is_plink:
        Z, miss = synth_genotypes(k, rows, seed=k + rows, missing_frac=0.02)
        X = np.ascontiguousarray(pack_plink(Z, miss))
    else:
        X = np.random.default_rng([k, rows]).integers(0, 256, (rows, (k + 3) // 4), dtype=np.uint8)
        X[:, -1] &= np.uint8((1 << (2 * (k % 4))) - 1)

    def run(A, device):
        to = _dev if device else (lambda a: a)
        M = to(np.full(rows * rows + 3, SENTINEL))
        assert L.snp_multiply_gpu(p(to(A)), k, rows, p(M), bool(is_plink)) == 0, mx.lib.last_error()
        M = _host(M)
        assert np.all(M[rows * rows:] == SENTINEL)
        out = [M[: rows * rows].reshape(rows, rows).copy()]
        cuts = [0, 256, rows] if rows > 256 else [0, rows]
        panels = []
        for c0, c1 in zip(cuts[:-1], cuts[1:]):                       # the column panels of the symmetric result, one guard column behind each
            Pn = to(np.full((c1 - c0 + 1, rows), SENTINEL))
            assert L.mxa_snp_multiply_panel(p(to(A)), k, rows, c0, c1, 0, p(Pn), rows, int(is_plink)) == 0, mx.lib.last_error()
            Pn = _host(Pn)
            assert np.all(Pn[c1 - c0] == SENTINEL)
            panels.append(Pn[: c1 - c0])
        out.append(np.concatenate(panels, axis=0))                    # row c of a panel = column c0 + c of the symmetric result
        return out

    clean = run(X, False)
    want = oracle.crossprod_i32(X, k, is_plink).astype(np.float64)
    assert np.array_equal(clean[0], want) and np.array_equal(clean[1], want)
    _same(run(X, True), clean, "device")
    for code, D in _patterns(X, k):
        want = oracle.crossprod_i32(D, k, is_plink).astype(np.float64)
        assert not np.array_equal(want, clean[0]), ("the oracle itself multiplies the padding", code)
        for device in (False, True):
            got = run(D, device)
            assert np.array_equal(got[0], want) and np.array_equal(got[1], want), (code, device)
            assert not np.array_equal(got[0], clean[0]), (code, device)
