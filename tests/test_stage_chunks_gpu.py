"""The three loops that bring a packed matrix from host memory or a .bed file to the device in row chunks -- recode_host_rows (mxa_stage.cpp), stage_operand
(mxa_crossprod.hip) and bed_range_to_handle (mxa_stage.cpp) -- run with more than one chunk.  MXA_STAGE_CHUNK_ROWS (read per call) sets the rows per chunk
in all three; every small shape of the suite otherwise runs them with exactly one chunk, so a second chunk (r0 > 0), the destination offsets row0 + r0,
dst_row0 + r and d_freq + r0, the reuse of the bounce buffer and of a pinned slot, and a has-3 / has-missing flag raised by a later chunk alone are not
executed there.

Main shape: 700 SNPs x 1027 individuals, 5 % missing codes.  SNP-major rows are 257 bytes (a ragged last byte, a partial ninth 32-byte slab),
individual-major rows 175 bytes.  Chunk sizes in rows: 1; 37 (boundaries inside a 32-row block of k_recode and inside a 256-row tile, a partial last chunk);
256 (a boundary exactly on a tile); rows - 1 (a last chunk of one row); rows and 100000 (one chunk, the clamp).

Chunks per call at the main shape:
    rows per chunk                                        1     37    256    699    700   100000
    recode_host_rows, 700 SNP-major rows                700     19      3      2      1        1
    recode_host_rows, 1027 individual-major rows       1027     28      5      2      2        1
    stage_operand, 700 rows (crossproduct, LD)          700     19      3      2      1        1
    stage_operand, 1027 rows (GRM)                     1027     28      5      2      2        1
    bed_range_to_handle, 700 rows (two pinned slots)    700     19      3      2      -        -

Every case compares the chunked host call (a) bit for bit with the same entry fed the same operands as device tensors, where no chunk loop runs, and
(b) with the independent reference the suite already uses for that entry, at that reference's tolerance: Oracle.dgemm_dense at 1e-11 max|ref| for products,
Oracle.crossprod_i32 / Oracle.allele_freq exactly, the dense GRM / LD maps of test_grm_ld_fused_gpu.py at 1e-12 / 1e-11, tests/_ld_ref.py within its bounds."""
import ctypes

import numpy as np
import pytest

import _ld_ref as ldr
import _operands as op
from _util import Oracle, make_B, make_problem

pytestmark = pytest.mark.gpu

SNPS, INDIV = 700, 1027
KNOB = "MXA_STAGE_CHUNK_ROWS"
RTOL = 1e-11                       # the fp64 products against Oracle.dgemm_dense
FEW = ("37", "1", "256")           # where a case does not run all six sizes


def chunk_sizes(rows):
    return ("1", "37", "256", str(rows - 1), str(rows), "100000")


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@pytest.fixture(scope="module")
def cache():
    """results of the device-in calls and the references, computed once and left unchanged"""
    return {}


def _on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _with_device_copies(prob):
    prob["plink_d"], prob["plink_t_d"] = _on_device(prob["plink"]), _on_device(prob["plink_t"])
    return prob


@pytest.fixture(scope="module")
def main(mx):
    prob = make_problem(SNPS, INDIV, 9, seed=SNPS + INDIV, missing_frac=0.05)
    assert prob["plink"].shape == (SNPS, 257) and prob["plink_t"].shape == (INDIV, 175)
    assert (ldr.codes(prob["plink"], INDIV) == 1).mean() > 0.04
    return _with_device_copies(prob)


def _env(monkeypatch, **kv):
    for k, v in kv.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def _operands(snps, indiv, ns=(1, 9), seed=5):
    """[(trans, B as make_B returns it: n rows of k values)]"""
    return [(t, make_B(indiv if t else snps, n, seed=seed + 2 * n + t)) for n in ns for t in (0, 1)]


def _products(dg, obj, snps, indiv, Bs):
    return [np.array(dg.dgemm_compressed_main(bool(t), obj, np.asfortranarray(B.T), snps, indiv)) for t, B in Bs]


def _assert_bits(got, want, what):
    assert len(got) == len(want), what
    for q, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(op.bits(a), op.bits(b)), (what, q)


def _assert_oracle(o, prob, Bs, Cs, what, centered=1):
    for (t, B), C in zip(Bs, Cs):
        m = prob["snps"] if t else prob["indiv"]
        ref = o.dgemm_dense(t, prob, B, centered)[:, :m]
        err = np.abs(C.T - ref).max() / np.abs(ref).max()
        assert err <= RTOL, (what, t, B.shape[0], err)


# ------------------------------------------------------------------------------------------------- a. plink2compressed from host pointers
@pytest.mark.parametrize("single", ["0", None])
@pytest.mark.parametrize("chunk", chunk_sizes(SNPS))
def test_plink2compressed_from_host_pointers(mx, monkeypatch, main, oracle, cache, single, chunk):
    """recode_host_rows for the SNP-major matrix and (MXA_SINGLE_ORIENTATION=0) for the individual-major one, against the object staged from device tensors"""
    dg = mx.dgemm_compressed
    dg.set_options(use_gpu=True, not_center=False, verbose=0)
    _env(monkeypatch, MXA_SINGLE_ORIENTATION=single, MIRACULIX_NUM_GPUS=None, **{KNOB: None})
    Bs = _operands(SNPS, INDIV)
    if ("a", single) not in cache:
        ref_obj = dg.init_compressed(main["plink_d"], main["plink_t_d"], SNPS, INDIV, main["f"], 9)
        try:
            cache[("a", single)] = _products(dg, ref_obj, SNPS, INDIV, Bs)
        finally:
            dg.free_compressed(ref_obj)
        _assert_oracle(oracle, main, Bs, cache[("a", single)], "device-in")
    monkeypatch.setenv(KNOB, chunk)
    obj = dg.init_compressed(main["plink"], main["plink_t"], SNPS, INDIV, main["f"], 9)
    try:
        assert dg.single_orientation(obj) == (0 if single == "0" else 1)
        Cs = _products(dg, obj, SNPS, INDIV, Bs)
    finally:
        dg.free_compressed(obj)
    _assert_bits(Cs, cache[("a", single)], ("host", single, chunk))
    _assert_oracle(oracle, main, Bs, Cs, ("host", single, chunk))


# --------------------------------------------------------------------------------------------------------------------------- b. shards
def test_shards_copy_the_individual_major_block_with_the_full_pitch(mx, monkeypatch, oracle):
    """MIRACULIX_NUM_GPUS=3 and mxa_plink2compressed_shard with two host pointers and two packed copies: the individual-major block of a shard has rows of
    ceil(rows of the shard / 4) bytes inside rows of ceil(1003 / 4) = 251 bytes, so every chunk is a pitched 2-D copy"""
    snps, indiv, n = 1003, INDIV, 4
    prob = _with_device_copies(make_problem(snps, indiv, n, seed=77, missing_frac=0.05))
    dg = mx.dgemm_compressed
    L = mx.lib.check_library_handle()
    dg.set_options(use_gpu=True, not_center=False, verbose=0)
    _env(monkeypatch, MXA_SINGLE_ORIENTATION="0", MIRACULIX_NUM_GPUS=None, **{KNOB: None})
    b, e = ctypes.c_long(-1), ctypes.c_long(-1)
    assert L.mxa_shard_bounds(snps, 3, 1, ctypes.byref(b), ctypes.byref(e)) == 3
    b, e = b.value, e.value
    assert 0 < b < e < snps and b % 4 == 0 and (e - b + 3) // 4 != (snps + 3) // 4
    mid = dict(snps=e - b, indiv=indiv, plink=np.ascontiguousarray(prob["plink"][b:e]), f=np.ascontiguousarray(prob["f"][b:e]))
    rng = np.random.default_rng(3)
    Bs = _operands(snps, indiv, ns=(n,))
    Bs_mid = _operands(e - b, indiv, ns=(n,))
    Bi = [(t, rng.integers(-50, 50, size=(n, indiv if t else snps)).astype(np.float64)) for t in (0, 1)]
    objs = []
    try:
        unsharded = dg.init_compressed(prob["plink_d"], prob["plink_t_d"], snps, indiv, prob["f"], n)
        objs.append(unsharded)
        shard_d = dg.init_compressed_shard(prob["plink_d"], prob["plink_t_d"], snps, indiv, b, e, prob["f"], n)
        objs.append(shard_d)
        monkeypatch.setenv("MIRACULIX_NUM_GPUS", "3")
        multi_d = dg.init_compressed(prob["plink_d"], prob["plink_t_d"], snps, indiv, prob["f"], n)
        objs.append(multi_d)
        want_multi = _products(dg, multi_d, snps, indiv, Bs)
        want_shard = _products(dg, shard_d, e - b, indiv, Bs_mid)
        dg.set_options(use_gpu=True, not_center=True, verbose=0)
        want_int = _products(dg, unsharded, snps, indiv, Bi)           # integer-valued B, uncentred: every sum is exact
        dg.set_options(use_gpu=True, not_center=False, verbose=0)
        for chunk in FEW:
            _env(monkeypatch, MIRACULIX_NUM_GPUS="3", **{KNOB: chunk})
            multi = dg.init_compressed(prob["plink"], prob["plink_t"], snps, indiv, prob["f"], n)
            objs.append(multi)
            assert dg.num_shards(multi) == 3 and dg.single_orientation(multi) == 0
            monkeypatch.delenv("MIRACULIX_NUM_GPUS")
            shard = dg.init_compressed_shard(prob["plink"], prob["plink_t"], snps, indiv, b, e, prob["f"], n)
            objs.append(shard)
            monkeypatch.delenv(KNOB)
            Cm = _products(dg, multi, snps, indiv, Bs)
            _assert_bits(Cm, want_multi, ("multi", chunk))
            _assert_oracle(oracle, prob, Bs, Cm, ("multi", chunk))
            Cs = _products(dg, shard, e - b, indiv, Bs_mid)
            _assert_bits(Cs, want_shard, ("shard", chunk))
            _assert_oracle(oracle, mid, Bs_mid, Cs, ("shard", chunk))
            dg.set_options(use_gpu=True, not_center=True, verbose=0)
            _assert_bits(_products(dg, multi, snps, indiv, Bi), want_int, ("multi, integer B", chunk))
            dg.set_options(use_gpu=True, not_center=False, verbose=0)
            for o_ in (multi, shard):
                dg.free_compressed(o_)
                objs.remove(o_)
    finally:
        dg.set_options(use_gpu=True, not_center=False, verbose=0)
        for o_ in objs:
            dg.free_compressed(o_)


# --------------------------------------------------------------------------------------------------------------- c. incremental staging
def test_appended_host_blocks_are_recoded_and_counted_chunk_by_chunk(mx, monkeypatch, main, oracle):
    """mxa_plink2compressed_rows with host blocks of 399, 300 and 1 rows, out of order, frequencies counted on the device: every chunk of a block writes its
    rows at snp_begin + r0 and its frequencies at d_f + snp_begin + r0"""
    dg = mx.dgemm_compressed
    dg.set_options(use_gpu=True, not_center=False, verbose=0)
    _env(monkeypatch, MXA_SINGLE_ORIENTATION=None, MIRACULIX_NUM_GPUS=None, **{KNOB: None})
    blocks = [(301, 700), (0, 300), (300, 301)]
    f_ref = oracle.allele_freq(main["plink"], SNPS, INDIV)
    counted = dict(main, f=f_ref)
    Bs = _operands(SNPS, INDIV)
    ref_obj = dg.init_compressed(main["plink_d"], None, SNPS, INDIV, f_ref, 9)
    try:
        want = _products(dg, ref_obj, SNPS, INDIV, Bs)
    finally:
        dg.free_compressed(ref_obj)
    _assert_oracle(oracle, counted, Bs, want, "init_compressed(plink, None, f_counted)")
    for chunk in (None, "1", "37", "256", "100000"):                   # None: device blocks, no chunk loop
        _env(monkeypatch, **{KNOB: chunk})
        src = main["plink_d"] if chunk is None else main["plink"]
        obj = dg.init_compressed_begin(SNPS, INDIV, 9)
        try:
            for b, e in blocks:
                dg.append_rows(obj, src[b:e], b, None)
            f = dg.init_compressed_end(obj, SNPS)
            Cs = _products(dg, obj, SNPS, INDIV, Bs)
        finally:
            dg.free_compressed(obj)
        assert np.array_equal(op.bits(f), op.bits(f_ref)), chunk
        _assert_bits(Cs, want, ("appended", chunk))


# ------------------------------------------------------------------------------------------------------------------------ d. dgemm_plink
def test_dgemm_plink_from_host_pointers(mx, monkeypatch, main, oracle):
    dg = mx.dgemm_compressed
    dg.set_options(use_gpu=True, not_center=False, verbose=0)
    _env(monkeypatch, MXA_SINGLE_ORIENTATION=None, MIRACULIX_NUM_GPUS=None, **{KNOB: None})
    for t in (0, 1):
        k, m = (INDIV, SNPS) if t else (SNPS, INDIV)
        B = make_B(k, 3, seed=11 + t)
        Bf = np.asfortranarray(B.T)
        for f in (main["f"], None):
            monkeypatch.delenv(KNOB, raising=False)
            want = np.array(dg.dgemm_plink(bool(t), main["plink_d"], main["plink_t_d"], SNPS, INDIV, f, Bf))
            ref = oracle.dgemm_dense(t, main, B, int(f is not None))[:, :m]
            assert np.abs(want.T - ref).max() <= RTOL * np.abs(ref).max(), (t, f is None)
            for chunk in FEW:
                monkeypatch.setenv(KNOB, chunk)
                got = np.array(dg.dgemm_plink(bool(t), main["plink"], main["plink_t"], SNPS, INDIV, f, Bf))
                _assert_bits([got], [want], ("dgemm_plink", t, f is None, chunk))


# ------------------------------------------------------------------------------------------------------------------ e. plain crossproduct
def _pack_fields(V):
    """rows of 2-bit values -> packed bytes, low bits first, zero padding"""
    rows, k = V.shape
    Vp = np.zeros((rows, (k + 3) // 4 * 4), np.uint8)
    Vp[:, :k] = V
    return np.ascontiguousarray(Vp[:, 0::4] | (Vp[:, 1::4] << 2) | (Vp[:, 2::4] << 4) | (Vp[:, 3::4] << 6))


def _set_code(X, row, j, code):
    """field j of a packed row := the 2-bit code"""
    s = 2 * (j % 4)
    X[row, j // 4] = (int(X[row, j // 4]) & ~(3 << s) & 0xFF) | (code << s)


def _crossprod_both_ways(mx, monkeypatch, oracle, cache, key, X, is_plink, engine, chunks):
    """snp_crossprod host in / host out at every chunk size == the device-in call == Oracle.crossprod_i32"""
    cp = mx.crossproduct
    _env(monkeypatch, MXA_XPROD_ENGINE=engine, **{KNOB: None})
    if (key, "ref") not in cache:
        cache[(key, "ref")] = oracle.crossprod_i32(X, INDIV, is_plink).astype(np.float64)
    ref = cache[(key, "ref")]
    if (key, engine) not in cache:
        cache[(key, engine)] = cp.snp_crossprod(_on_device(X), SNPS, INDIV, is_snpmajor=True, is_plink_format=is_plink).cpu().numpy()
        assert np.array_equal(cache[(key, engine)], ref), (key, engine, "device-in")
    for chunk in chunks:
        monkeypatch.setenv(KNOB, chunk)
        M = cp.snp_crossprod(X, SNPS, INDIV, is_snpmajor=True, is_plink_format=is_plink)
        assert np.array_equal(M, ref), (key, engine, chunk)
        _assert_bits([M], [cache[(key, engine)]], (key, engine, chunk))
    return ref


@pytest.mark.parametrize("engine", [None, "i8"])
@pytest.mark.parametrize("chunk", chunk_sizes(SNPS))
def test_plain_crossproduct_from_a_host_matrix(mx, monkeypatch, main, oracle, cache, engine, chunk):
    """stage_operand -> k_xstage without the field mask: the PLINK table (bytes with a missing pair read as four 3s), and raw fields with the value 3"""
    if "raw" not in cache:
        cache["raw"] = _pack_fields(np.random.default_rng(12).integers(0, 4, size=(SNPS, INDIV)).astype(np.uint8))
    _crossprod_both_ways(mx, monkeypatch, oracle, cache, "e-plink", main["plink"], True, engine, (chunk,))
    ref = _crossprod_both_ways(mx, monkeypatch, oracle, cache, "e-raw", cache["raw"], False, engine, (chunk,))
    assert ref.max() > 4 * INDIV * 0.4                                                       # the 3s are there


@pytest.mark.parametrize("engine", [None, "i8"])
def test_has3_flag_raised_by_the_last_chunk_alone(mx, monkeypatch, oracle, cache, engine):
    """a PLINK matrix whose only missing code is in its last row: only the last chunk raises the flag, and the byte still counts as four 3s"""
    X = make_problem(SNPS, INDIV, 1, seed=5)["plink"].copy()
    assert not (ldr.codes(X, INDIV) == 1).any()
    j = 513
    _set_code(X, SNPS - 1, j, 1)
    assert np.argwhere(ldr.codes(X, INDIV) == 1).tolist() == [[SNPS - 1, j]]
    ref = _crossprod_both_ways(mx, monkeypatch, oracle, cache, "e-last", X, True, engine, FEW)
    Zs = ldr.staged(X, True).astype(np.int64)                                                # the byte table restated in numpy
    assert (Zs[SNPS - 1, j // 4 * 4: j // 4 * 4 + 4] == 3).all() and (Zs == 3).sum() == 4
    assert np.array_equal(ref, (Zs @ Zs.T).astype(np.float64))


# ------------------------------------------------------------------------------------------------- f. GRM and LD from host matrices
def _grm_map(M, f, do_scale):
    """crossproduct.jl:96-107 on a given crossproduct M (the dense restatement of tests/test_grm_ld_fused_gpu.py)"""
    n = M.shape[0]
    cs = M.sum(axis=0)
    M = M - np.outer(cs, np.ones(n)) / n - np.outer(np.ones(n), cs) / n + cs.sum() / n ** 2
    return M / (2 * np.sum(f * (1 - f))) if do_scale else M


def _ld_map(M, f, indiv):
    """crossproduct.jl:139-149 on a given crossproduct M (tests/test_grm_ld_fused_gpu.py)"""
    M = M - 4.0 * indiv * np.outer(f, f)
    s = np.sqrt(np.diag(M))
    return M / s[:, None] / s[None, :]


@pytest.mark.parametrize("chunk", chunk_sizes(SNPS))
def test_grm_and_ld_from_host_matrices_with_dirty_padding(mx, monkeypatch, main, oracle, cache, chunk):
    """stage_operand -> k_xstage WITH the field mask.  SNP-major rows hold 1027 fields in 257 bytes: their one padding field is filled with a per-row pick of
    01 / 10 / 11 and must be staged as 00 in every chunk.  The GRM reads that matrix with its axes exchanged (700 "individuals" of 1027 "SNPs": padding
    fields) and the individual-major matrix as it is (1027 rows of 700 fields: no padding field, five tiles)."""
    cp = mx.crossproduct
    _env(monkeypatch, MXA_XPROD_ENGINE=None, MXA_XPROD_FUSED_POST=None, **{KNOB: None})
    if "f" not in cache:
        Xd = op.dirty(main["plink"], INDIV, "random")
        assert op.padding_fields(INDIV) == 1 and not np.array_equal(Xd, main["plink"])
        f2 = np.random.default_rng(4).uniform(0.1, 0.5, size=INDIV)
        M_s = oracle.crossprod_i32(main["plink"], INDIV, True).astype(np.float64)            # of the CLEAN rows: padding bits are no data
        M_i = oracle.crossprod_i32(main["plink_t"], SNPS, True).astype(np.float64)
        calls = {}
        for do_scale in (True, False):
            calls[("grm-x", do_scale)] = (lambda X, s=do_scale: cp.grm(X, INDIV, SNPS, is_plink_format=True, do_scale=s, allele_freq=f2 if s else None),
                                          Xd, _grm_map(M_s, f2, do_scale), 1e-12)
            calls[("grm", do_scale)] = (lambda X, s=do_scale: cp.grm(X, SNPS, INDIV, is_plink_format=True, do_scale=s, allele_freq=main["f"] if s else None),
                                        main["plink_t"], _grm_map(M_i, main["f"], do_scale), 1e-12)
        calls["ld"] = (lambda X: cp.ld(X, SNPS, INDIV, is_plink_format=True, allele_freq=main["f"]), Xd, _ld_map(M_s, main["f"], INDIV), None)
        want = {}
        for key, (call, X, ref, rtol) in calls.items():
            want[key] = call(_on_device(X)).cpu().numpy()
            if rtol is None:                                                                 # LD: 1e-11 absolute on the finite entries
                assert np.isfinite(ref).all() and np.isfinite(want[key]).all()
                assert np.abs(want[key] - ref).max() <= 1e-11, key
            else:
                assert np.abs(want[key] - ref).max() <= rtol * np.abs(ref).max(), key
        cache["f"] = (calls, want)
    calls, want = cache["f"]
    monkeypatch.setenv(KNOB, chunk)
    for key, (call, X, ref, rtol) in calls.items():
        got = call(X)
        _assert_bits([got], [want[key]], (key, chunk))
        assert np.abs(got - ref).max() <= (1e-11 if rtol is None else rtol * np.abs(ref).max()), (key, chunk)


# ----------------------------------------------------------------------------------------------- g. windowed LD from a host matrix
G_SNPS, G_INDIV, G_WINDOW = 700, 259, 300


def _band_of(R, window):
    """(out[i, d] = R[i, i + d], the mask of the entries with i + d < snps)"""
    n = R.shape[0]
    idx = np.arange(n)[:, None] + np.arange(window + 1)[None, :]
    return R[np.arange(n)[:, None], np.minimum(idx, n - 1)], idx < n


def _ld_entries(cp, X, f, Xapply):
    """every windowed-LD entry that stages the packed matrix X (numpy: through the chunk loop; device tensor: in place), results as numpy"""
    snps, indiv, w = G_SNPS, G_INDIV, G_WINDOW
    last = ldr.fixed_last(snps, w)
    back = op.readback
    out = {}
    out["band"] = back(cp.ld_band(X, snps, indiv, w, kind="r", is_plink_format=True, allele_freq=f))
    out["band pairwise"] = back(cp.ld_band_pairwise(X, snps, indiv, w, kind="r"))
    out["scores"] = back(cp.ld_window_scores(X, snps, indiv, last, adjust=False, is_plink_format=True, allele_freq=f))
    out["scores pairwise"] = back(cp.ld_window_scores_pairwise(X, snps, indiv, last, adjust=True))
    rowptr, col, val = cp.ld_pairs(X, snps, indiv, window=w, min_r2=0.01, kind="r", is_plink_format=True, allele_freq=f)
    out["pairs rowptr"], out["pairs col"], out["pairs val"] = back(rowptr), back(col), back(val)
    for pairwise in (False, True):
        with cp.LdOperator.create(X, snps, indiv, window=w, kind="r", pairwise=pairwise, is_plink_format=True, allele_freq=None if pairwise else f) as T:
            tag = "operator pairwise" if pairwise else "operator"
            out[tag + " rows"] = back(T.rows())
            out[tag + " apply"] = back(T.apply(Xapply))
    return out


def _assert_pairwise_band(got, r_ref, window, what):
    want, inband = _band_of(r_ref, window)
    assert np.array_equal(np.isnan(got) & inband, np.isnan(want) & inband), what
    ok = inband & ~np.isnan(want)
    err = np.abs(got.astype(ldr.LD) - want)[ok].astype(np.float64)
    assert np.all(err <= ldr.pairwise_bound(want)[ok]), (what, float(err.max()))


@pytest.mark.parametrize("chunk", chunk_sizes(G_SNPS))
def test_windowed_ld_from_a_host_matrix(mx, monkeypatch, cache, chunk):
    """stage_operand -> k_xstage with the mask (the plain entries) and -> k_xstage_planes (the pairwise entries): 700 SNPs in three tiles, rows of 65 bytes
    with one padding field, window 300 (every band tile of three tile rows)"""
    cp = mx.crossproduct
    _env(monkeypatch, MXA_XPROD_ENGINE=None, MXA_LD_PAIRWISE_SCRATCH_MB=None, MXA_LD_PAIRWISE_DENSE=None, **{KNOB: None})
    if "g" not in cache:
        prob = make_problem(G_SNPS, G_INDIV, 1, seed=G_SNPS + G_INDIV, missing_frac=0.05)
        X, f = prob["plink"], prob["f"]
        assert X.shape == (G_SNPS, 65) and (ldr.codes(X, G_INDIV) == 1).any()
        Xapply = np.random.default_rng(8).standard_normal((G_SNPS, 3))
        want = _ld_entries(cp, _on_device(X), f, Xapply)
        case = ldr.plain_case(X, G_INDIV, f)
        (r, inband), (b, _) = _band_of(case["r"], G_WINDOW), _band_of(case["b"], G_WINDOW)
        assert np.isfinite(b[inband]).all()
        ratio = ldr.worst_ratio(want["band"][inband], r[inband], b[inband])
        print(f"windowed LD, plain band: worst |r - r_ref| / bound = {ratio:.3f}")
        assert ratio <= 1.0, ratio
        assert np.all(want["band"][~inband] == 0.0)
        _assert_pairwise_band(want["band pairwise"], ldr.pairwise_restate(X, G_INDIV)["r"], G_WINDOW, "device-in")
        assert len(want["pairs col"]) > G_SNPS and want["pairs rowptr"][-1] == len(want["pairs col"])
        cache["g"] = (X, f, Xapply, want, (r, b, inband))
    X, f, Xapply, want, (r, b, inband) = cache["g"]
    monkeypatch.setenv(KNOB, chunk)
    got = _ld_entries(cp, X, f, Xapply)
    assert sorted(got) == sorted(want)
    for key in want:
        _assert_bits([got[key]], [want[key]], (key, chunk))
    assert ldr.worst_ratio(got["band"][inband], r[inband], b[inband]) <= 1.0


def test_pairwise_ld_with_the_only_missing_call_in_the_last_chunk(mx, monkeypatch):
    """k_xstage_planes raises *has_missing; without it the entry takes the complete-data route.  One missing call, in the last SNP: with 37, 1 or 256 rows per
    chunk only the last chunk sees it, and the result must still be the pairwise-complete r"""
    cp = mx.crossproduct
    _env(monkeypatch, MXA_XPROD_ENGINE=None, MXA_LD_PAIRWISE_SCRATCH_MB=None, MXA_LD_PAIRWISE_DENSE=None, **{KNOB: None})
    snps, indiv, w = G_SNPS, G_INDIV, G_WINDOW
    X = make_problem(snps, indiv, 1, seed=19)["plink"].copy()
    assert not (ldr.codes(X, indiv) == 1).any()
    j = 100
    X0 = X.copy()                                                                            # complete data: the call read as allele count 0
    _set_code(X0, snps - 1, j, 0)
    _set_code(X, snps - 1, j, 1)
    assert np.argwhere(ldr.codes(X, indiv) == 1).tolist() == [[snps - 1, j]]
    r_pw, r_cd = ldr.pairwise_restate(X, indiv)["r"], ldr.pairwise_restate(X0, indiv)["r"]
    # the two references differ at that SNP by far more than the bound, so the complete-data result cannot pass as the pairwise-complete one
    col = slice(snps - 1 - w, snps - 1)
    gap = np.abs(r_pw[col, snps - 1] - r_cd[col, snps - 1]).astype(np.float64)
    assert np.all(np.isfinite(gap)) and (gap > 100 * ldr.pairwise_bound(r_pw[col, snps - 1])).sum() > w // 2
    last = ldr.fixed_last(snps, w)
    Xd = _on_device(X)
    want_band = cp.ld_band_pairwise(Xd, snps, indiv, w, kind="r").cpu().numpy()
    want_scores = cp.ld_window_scores_pairwise(Xd, snps, indiv, last, adjust=False).cpu().numpy()
    _assert_pairwise_band(want_band, r_pw, w, "device-in")
    for chunk in FEW:
        monkeypatch.setenv(KNOB, chunk)
        band = cp.ld_band_pairwise(X, snps, indiv, w, kind="r")
        _assert_pairwise_band(band, r_pw, w, chunk)
        _assert_bits([band, cp.ld_window_scores_pairwise(X, snps, indiv, last, adjust=False)], [want_band, want_scores], ("pairwise", chunk))


# ------------------------------------------------------------------------------------------------------------------------------ h. .bed
def _write_bed(mx, tmp_path, plink):
    bed = str(tmp_path / "chunks.bed")
    mx.read_plink.write_bed(bed, plink)
    return bed


@pytest.mark.parametrize("single", ["1", "0"])
def test_bed_file_in_three_or_more_chunks(mx, monkeypatch, main, oracle, tmp_path, single):
    """bed_range_to_handle, streaming into a one-copy object (MXA_SINGLE_ORIENTATION=1: upload, k_recode at row r0 and k_allele_freq at d_f + r0 per chunk) and
    raw block + transpose for a two-copy object (=0: upload at d_plink + r0 * bps).  1, 37 and 256 rows per chunk give 700, 19 and 3 chunks: both pinned slots
    are reused after their events; 699 gives a last chunk of one row."""
    dg = mx.dgemm_compressed
    dg.set_options(use_gpu=True, not_center=False, verbose=0)
    _env(monkeypatch, MXA_SINGLE_ORIENTATION=single, MIRACULIX_NUM_GPUS=None, **{KNOB: None})
    bed = _write_bed(mx, tmp_path, main["plink"])
    f_ref = oracle.allele_freq(main["plink"], SNPS, INDIV)
    counted = dict(main, f=f_ref)
    Bs = _operands(SNPS, INDIV, ns=(4,))
    ref_obj = dg.init_compressed(main["plink_d"], None, SNPS, INDIV, f_ref, 4)
    try:
        want = _products(dg, ref_obj, SNPS, INDIV, Bs)
    finally:
        dg.free_compressed(ref_obj)
    for chunk in ("1", "37", "256", str(SNPS - 1)):
        monkeypatch.setenv(KNOB, chunk)
        obj, f, s_out, i_out = dg.init_compressed_from_bed(bed, 4, snps=SNPS, indiv=INDIV)
        try:
            assert (s_out, i_out) == (SNPS, INDIV) and dg.single_orientation(obj) == int(single)
            Cs = _products(dg, obj, SNPS, INDIV, Bs)
        finally:
            dg.free_compressed(obj)
        assert np.array_equal(op.bits(f), op.bits(f_ref)), chunk
        _assert_bits(Cs, want, (".bed", single, chunk))
        _assert_oracle(oracle, counted, Bs, Cs, (".bed", single, chunk))


# ------------------------------------------------------------------------------------------------------------ i. .bed ranges and shards
@pytest.mark.parametrize("single", [None, "0"])
def test_bed_ranges_and_shards_in_chunks(mx, monkeypatch, main, oracle, tmp_path, single):
    """mxa_bed2compressed_range for [0, 1), [699, 700) and [5, 262) (ends that are multiples of neither 4 nor 256), and the in-process sharder over the same
    file: frequencies = the slice of the oracle's, products = those of the object staged from the same rows in device memory"""
    dg = mx.dgemm_compressed
    dg.set_options(use_gpu=True, not_center=False, verbose=0)
    _env(monkeypatch, MXA_SINGLE_ORIENTATION=single, MIRACULIX_NUM_GPUS=None, **{KNOB: None})
    bed = _write_bed(mx, tmp_path, main["plink"])
    f_ref = oracle.allele_freq(main["plink"], SNPS, INDIV)
    n = 4
    for b, e in ((0, 1), (SNPS - 1, SNPS), (5, 262)):
        Bs = _operands(e - b, INDIV, ns=(n,))
        part = dict(snps=e - b, indiv=INDIV, plink=np.ascontiguousarray(main["plink"][b:e]), f=np.ascontiguousarray(f_ref[b:e]))
        monkeypatch.delenv(KNOB, raising=False)
        ref_obj = dg.init_compressed(main["plink_d"][b:e], None, e - b, INDIV, part["f"], n)
        try:
            want = _products(dg, ref_obj, e - b, INDIV, Bs)
        finally:
            dg.free_compressed(ref_obj)
        _assert_oracle(oracle, part, Bs, want, ("rows in memory", b, e))
        for chunk in FEW:
            monkeypatch.setenv(KNOB, chunk)
            obj, f = dg.init_compressed_from_bed_range(bed, b, e, n, snps=SNPS, indiv=INDIV)
            try:
                Cs = _products(dg, obj, e - b, INDIV, Bs)
            finally:
                dg.free_compressed(obj)
            assert np.array_equal(op.bits(f), op.bits(part["f"])), (b, e, chunk)
            _assert_bits(Cs, want, ("range", b, e, single, chunk))
    # MIRACULIX_NUM_GPUS=3 from the same file against the sharded object staged from device memory
    Bs = _operands(SNPS, INDIV, ns=(n,))
    counted = dict(main, f=f_ref)
    _env(monkeypatch, MIRACULIX_NUM_GPUS="3", **{KNOB: None})
    ref_obj = dg.init_compressed(main["plink_d"], None, SNPS, INDIV, f_ref, n)
    try:
        assert dg.num_shards(ref_obj) == 3
        want = _products(dg, ref_obj, SNPS, INDIV, Bs)
    finally:
        dg.free_compressed(ref_obj)
    for chunk in FEW:
        monkeypatch.setenv(KNOB, chunk)
        obj, f, _, _ = dg.init_compressed_from_bed(bed, n, snps=SNPS, indiv=INDIV)
        try:
            assert dg.num_shards(obj) == 3
            Cs = _products(dg, obj, SNPS, INDIV, Bs)
        finally:
            dg.free_compressed(obj)
        assert np.array_equal(op.bits(f), op.bits(f_ref)), chunk
        _assert_bits(Cs, want, ("sharded .bed", single, chunk))
        _assert_oracle(oracle, counted, Bs, Cs, ("sharded .bed", single, chunk))


# ------------------------------------------------------------------------------------------------------------------- j. the knob itself
def test_values_that_are_no_positive_integer_mean_the_default(mx, monkeypatch, main, oracle, tmp_path):
    """The empty string, "0", "-3" and "abc": each of the three loops runs with its default chunk and gives the same bits; so does a call after the variable is removed"""
    dg, cp = mx.dgemm_compressed, mx.crossproduct
    dg.set_options(use_gpu=True, not_center=False, verbose=0)
    _env(monkeypatch, MXA_SINGLE_ORIENTATION=None, MIRACULIX_NUM_GPUS=None, MXA_XPROD_ENGINE=None, **{KNOB: None})
    bed = _write_bed(mx, tmp_path, main["plink"])
    Bs = _operands(SNPS, INDIV, ns=(2,))

    def run():
        out = [cp.snp_crossprod(main["plink"], SNPS, INDIV, is_snpmajor=True, is_plink_format=True)]
        obj = dg.init_compressed(main["plink"], None, SNPS, INDIV, main["f"], 2)
        try:
            out += _products(dg, obj, SNPS, INDIV, Bs)
        finally:
            dg.free_compressed(obj)
        obj, f, _, _ = dg.init_compressed_from_bed(bed, 2, snps=SNPS, indiv=INDIV)
        try:
            out += [f] + _products(dg, obj, SNPS, INDIV, Bs)
        finally:
            dg.free_compressed(obj)
        return out

    want = run()
    assert np.array_equal(want[0], oracle.crossprod_i32(main["plink"], INDIV, True).astype(np.float64))
    for value in ("", "0", "-3", "abc", "37"):
        monkeypatch.setenv(KNOB, value)
        _assert_bits(run(), want, repr(value))
    monkeypatch.delenv(KNOB)
    _assert_bits(run(), want, "after delenv")
