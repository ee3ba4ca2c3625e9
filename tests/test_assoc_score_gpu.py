"""mxa_assoc_score on the device.  The exact family (tests/_assoc_score_ref.py: every sum the definition names is exact in fp64) bit for bit against the
documented chain, NaN positions included, over the shapes at which the scan, the product and the weight kernel change path; real data (the null model fitted
by mxa_assoc_logistic_null) against the long-double evaluation of the definition within 4 x its first-order forward bound, and against the textbook form with
an explicit (C^T W C)^-1; identity of the bits between pointer kinds, layouts, alignments, staging chunks, runs and the process-wide centring option.

Shapes: indiv in {19, 67, 259, 1027} (partial last bytes; the 16-byte word edges), snps in {1, 7, 33} and {15, 16, 17} (the weight kernel tiles 16 SNP rows),
(n, kh) with n (kh + 2) columns of B on both sides of the scan's 16 and the product's 32 ((1, 14), (1, 15), (2, 15)), n = 17 (seventeen
passes of the weight kernel, one column each), kh = 0.  Long rows, indiv in {16387, 65539} (257 and 1025 words of 64 genotypes: threads of the weight kernel and of the scan loop), with 9 SNPs."""
import functools
import itertools

import numpy as np
import pytest

import _assoc_score_ref as sr
import _operands as op

pytestmark = pytest.mark.gpu

SENTINEL = -7.5
SEED = 5
MEMBERS = ((19, 1, 1), (19, 2, 3), (67, 3, 4), (259, 1, 16), (259, 17, 2), (1027, 2, 17))
ROW_TILE = 16          # kScoreRows of mxa_assoc.hip


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def exact_case(indiv, snps, n, kh, missing=0.05):
    """(codes, packed rows, R, Wt, H, (score, var, z, nobs) of the chain): computed once, shared, read-only.  The reference V is positive on every ordinary
    row -- every row but the six edge patterns of genotypes(...) -- so that NaN == NaN cannot hide a failure."""
    R, Wt, H = sr.score_family(indiv, n, kh, SEED)
    codes = sr.genotypes(snps, indiv, seed=SEED, missing=missing, special=missing > 0)
    want = sr.chain_score(codes, R, Wt, H)
    first = 6 if (snps >= 7 and missing > 0) else 0
    assert np.all(want[1][first:] > 0) and np.all(np.isfinite(want[2][first:])), (indiv, snps, n, kh)
    _frozen(codes, R, Wt, H, *want)
    return codes, sr.pack(codes), R, Wt, H, want


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")          # (a copy: the shared cases are read-only)


def _columns(M, ld, device, fill=np.nan):
    """the column-major operand of M (rows, cols) with leading dimension ld (the rows behind a column hold `fill`), on the host or the device"""
    rows, cols = M.shape
    buf = np.full((max(cols, 1), ld), fill)
    buf[:cols, :rows] = M.T
    return _dev(buf) if device else buf


def run(mx, plink, snps, indiv, R, Wt, H, dev=(False,) * 5, ld=(None,) * 4, want=(True, True, True), nobs_dev=False, operands=None):
    """one call through the C ABI; dev: plink, R, Wt, H, results on the device; ld: ldr, ldw, ldh, ldo.  Returns (score, var, z) as (snps, n) arrays (None where
    not wanted) and nobs, after checking that nothing beyond row snps - 1 of a column or beyond column n - 1 was written."""
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    n = R.shape[1]
    kh = H.shape[1] // n
    ldr, ldw, ldh, ldo = ld[0] or indiv, ld[1] or indiv, ld[2] or indiv, ld[3] or snps
    if operands is None:
        operands = (_dev(plink) if dev[0] else np.ascontiguousarray(plink), _columns(R, ldr, dev[1]), _columns(Wt, ldw, dev[2]), _columns(H, ldh, dev[3]) if kh else None)
    P, rb, wb, hb = operands
    res = [(_dev(np.full((n + 1, ldo), SENTINEL)) if dev[4] else np.full((n + 1, ldo), SENTINEL)) if w else None for w in want]
    nobs = _dev(np.full(snps + 1, -3, np.int32)) if nobs_dev else np.full(snps + 1, -3, np.int32)
    rc = L.mxa_assoc_score(p(P), snps, indiv, p(rb), ldr, p(wb), ldw, p(hb), ldh, n, kh, p(res[0]), p(res[1]), p(res[2]), ldo, p(nobs))
    assert rc == 0, mx.lib.last_error()
    outs = []
    for r in res:
        if r is None:
            outs.append(None)
            continue
        r = op.readback(r)
        assert np.all(r[n] == SENTINEL) and np.all(r[:, snps:] == SENTINEL)
        outs.append(np.ascontiguousarray(r[:n, :snps].T))
    nobs = op.readback(nobs)
    assert nobs[snps] == -3
    return outs, nobs[:snps]


def check_exact(got, nobs, want):
    for name, g, w in zip(("score", "var", "z"), got, want[:3]):
        if g is not None:
            assert sr.same_bits(g, w), (name, np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))[:5])
    assert np.array_equal(nobs, want[3])


def run_case(mx, case, **kw):
    codes, P, R, Wt, H, want = case
    got, nobs = run(mx, P, codes.shape[0], codes.shape[1], R, Wt, H, **kw)
    check_exact(got, nobs, want)
    return got


@pytest.mark.parametrize("snps", (1, 7, 33))
@pytest.mark.parametrize("indiv, n, kh", MEMBERS)
def test_exact_family_bit_for_bit(mx, indiv, snps, n, kh):
    case = exact_case(indiv, snps, n, kh)
    codes = case[0]
    if snps >= 7:       # the patterns are there: N = 0, one called individual, constant on the called, a missing code in the last field, no missing code
        assert np.all(codes[0] < 0) and (codes[1] >= 0).sum() == 1 and codes[4, -1] < 0 and not np.any(codes[5] < 0) and (snps < 33 or np.any(codes[6:] < 0))
    else:               # ordinary rows: the SNPs compare finite bits
        assert np.all(np.isfinite(case[5][2]))
    got = run_case(mx, case)
    if snps >= 7:
        assert np.all(np.isnan(got[2][0])) and np.all(np.isfinite(got[2][6:]))


@pytest.mark.parametrize("indiv, snps, n, kh", [(67, 33, 1, 14), (67, 33, 1, 15), (67, 33, 2, 15),                      # 16, 17 and 34 columns of B
                                                 (67, ROW_TILE - 1, 3, 4), (67, ROW_TILE, 3, 4), (67, ROW_TILE + 1, 3, 4),  # the weight kernel's row tile
                                                 (67, 33, 2, 0), (19, 7, 1, 0), (259, 33, 5, 0)])                             # no projection column
def test_exact_family_at_the_column_and_row_tile_edges(mx, indiv, snps, n, kh):
    run_case(mx, exact_case(indiv, snps, n, kh))
    run_case(mx, exact_case(indiv, snps, n, kh), dev=(True,) * 5)


@pytest.mark.parametrize("indiv", [16387, 65539])
def test_exact_family_long_rows_bit_for_bit(mx, indiv):
    """rows of more than 256 and more than 512 logical words: threads of the weight kernel take a second word, and every thread of the scan loops.  Nine SNPs (the six edge
    patterns and three ordinary rows); host and device pointers; the 4097- and 16385-byte rows start at every offset of a 16-byte word, and once more from
    a base one byte off a 64-byte boundary"""
    snps, n, kh = 9, 2, 3
    case = exact_case(indiv, snps, n, kh)
    assert (indiv + 3) // 4 > 256 * 16 and np.any(case[0][6:] < 0)
    for dev in (False, True):
        run_case(mx, case, dev=(dev,) * 5)
        P, _ = op.misaligned(case[1], 1, dev)
        got, nobs = run(mx, None, snps, indiv, case[2], case[3], case[4],
                        operands=(P, _columns(case[2], indiv, dev), _columns(case[3], indiv, dev), _columns(case[4], indiv, dev)))
        check_exact(got, nobs, case[5])


@pytest.mark.parametrize("indiv, n, kh", MEMBERS)
def test_exact_family_without_any_missing_code(mx, indiv, n, kh):
    """no 01 field anywhere: the scan skips its further column chunks, M must still be zero and E must still be right"""
    case = exact_case(indiv, 33, n, kh, missing=0.0)
    assert not np.any(case[0] < 0) and np.any(case[0] == 2)
    run_case(mx, case, dev=(True, False, False, False, True))
    assert np.all(case[5][3] == indiv)


def test_only_missing_codes(mx):
    indiv, snps, n, kh = 67, 17, 2, 3
    R, Wt, H = sr.score_family(indiv, n, kh, SEED)
    codes = np.full((snps, indiv), -1, np.int8)
    want = sr.chain_score(codes, R, Wt, H)
    assert np.all(np.isnan(want[0])) and np.all(np.isnan(want[1])) and np.all(want[3] == 0)
    for dev in (False, True):
        got, nobs = run(mx, sr.pack(codes), snps, indiv, R, Wt, H, dev=(dev,) * 5)
        check_exact(got, nobs, want)


@pytest.mark.parametrize("indiv", [19, 67, 259, 1027])
def test_rows_whose_only_11_is_the_last_individual_and_11_in_the_padding(mx, indiv):
    """E of a row is the last individual's weight alone, whatever the padding fields hold; and rows without any 11 among the individuals keep E = 0 with 11
    patterns in every padding field"""
    snps, n, kh = 18, 3, 2
    R, Wt, H = sr.score_family(indiv, n, kh, SEED)
    rng = np.random.default_rng([SEED, indiv, 9])
    codes = rng.choice(np.array([-1, 0, 1], np.int8), size=(snps, indiv), p=[0.05, 0.55, 0.4])
    codes[::2, -1] = 2
    want = sr.chain_score(codes, R, Wt, H)
    assert op.padding_fields(indiv) > 0 and np.all(want[1] > 0)
    P = sr.pack(codes)
    for plink in (P, op.dirty(P, indiv, 3), op.dirty(P, indiv, "random")):
        for dev in (False, True):
            got, nobs = run(mx, plink, snps, indiv, R, Wt, H, dev=(dev, False, False, False, False))
            check_exact(got, nobs, want)


def test_host_and_device_pointers_in_every_combination(mx):
    case = exact_case(67, 33, 3, 4)
    for dev in itertools.product((False, True), repeat=5):
        run_case(mx, case, dev=dev, nobs_dev=dev[0])
    # mixed host and device result pointers are refused, nothing is written
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    snps, indiv, n, kh = 33, 67, 3, 4
    h, d = np.full((n, snps), SENTINEL), _dev(np.full((n, snps), SENTINEL))
    rc = L.mxa_assoc_score(p(np.ascontiguousarray(case[1])), snps, indiv, p(_columns(case[2], indiv, False)), indiv, p(_columns(case[3], indiv, False)), indiv,
                           p(_columns(case[4], indiv, False)), indiv, n, kh, p(h), p(d), None, snps, None)
    assert rc == 1 and L.mxa_last_error() == 1 and np.all(h == SENTINEL) and np.all(op.readback(d) == SENTINEL)


@pytest.mark.parametrize("dev", [False, True])
def test_leading_dimensions_larger_than_needed_and_optional_outputs(mx, dev):
    case = exact_case(259, 33, 1, 16)
    snps, indiv = 33, 259
    run_case(mx, case, dev=(dev,) * 5, ld=(indiv + 3, indiv + 1, indiv + 2, snps + 5))
    for want in ((False, True, True), (True, False, True), (True, True, False), (False, False, True), (True, False, False)):
        got = run_case(mx, case, dev=(dev,) * 5, want=want, ld=(None, None, None, snps + 1))
        assert [g is not None for g in got] == list(want)
    # nobs is optional too
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    z = np.full((1, snps), SENTINEL)
    assert L.mxa_assoc_score(p(np.ascontiguousarray(case[1])), snps, indiv, p(_columns(case[2], indiv, False)), indiv, p(_columns(case[3], indiv, False)), indiv,
                             p(_columns(case[4], indiv, False)), indiv, 1, 16, None, None, p(z), snps, None) == 0
    assert sr.same_bits(z.T, case[5][2])


@pytest.mark.parametrize("indiv", [19, 67, 259, 1027])
def test_dirty_padding_fields_give_the_same_bits(mx, indiv):
    case = exact_case(indiv, 33, 2, 3)
    assert op.padding_fields(indiv) > 0
    for code in op.CODES:
        for dev in (False, True):
            got, nobs = run(mx, op.dirty(case[1], indiv, code), 33, indiv, case[2], case[3], case[4], dev=(dev, False, False, False, False))
            check_exact(got, nobs, case[5])


@pytest.mark.parametrize("device", [False, True])
def test_pointers_off_a_64_byte_and_a_16_byte_boundary_give_the_same_bits(mx, device):
    indiv, snps, n, kh = 259, 33, 3, 4          # 65-byte rows: the rows start at every offset of a 16-byte word
    case = exact_case(indiv, snps, n, kh)
    plain = [_columns(case[i], indiv, False) for i in (2, 3, 4)]
    for off in op.BYTE_OFFSETS + (16, 17):
        P, _ = op.misaligned(case[1], off, device)
        got, nobs = run(mx, None, snps, indiv, case[2], case[3], case[4], operands=(P,) + tuple(_dev(b) if device else b for b in plain))
        check_exact(got, nobs, case[5])
    for off in op.WIDE_OFFSETS + (2, 3):        # 8, 16 and 24 bytes off a 64-byte boundary
        moved = tuple(op.misaligned(b, off, device)[0] for b in plain)
        got, nobs = run(mx, None, snps, indiv, case[2], case[3], case[4], operands=(_dev(case[1]) if device else np.ascontiguousarray(case[1]),) + moved)
        check_exact(got, nobs, case[5])


def test_a_small_staging_chunk_two_runs_and_the_centring_option_give_the_same_bits(mx, monkeypatch):
    """MXA_ASSOC_CHUNK_ROWS = 5: a host matrix staged in chunks of five rows (the last one partial; every chunk smaller than the weight kernel's row tile); a
    second run; setOptions_compressed with centring off and on.  The test ends with centring on, the library's state before any setOptions_compressed call."""
    dg = mx.dgemm_compressed
    for indiv, snps, n, kh in ((259, 33, 17, 2), (67, 33, 3, 4)):
        case = exact_case(indiv, snps, n, kh)
        first = run_case(mx, case)
        monkeypatch.setenv("MXA_ASSOC_CHUNK_ROWS", "5")
        again = run_case(mx, case)
        monkeypatch.delenv("MXA_ASSOC_CHUNK_ROWS")
        assert all(np.array_equal(op.bits(a), op.bits(b)) for a, b in zip(first, again))
        for not_center in (True, False):
            dg.set_options(use_gpu=True, not_center=not_center, verbose=0)
            for dev in (False, True):
                again = run_case(mx, case, dev=(dev,) * 5)
                assert all(np.array_equal(op.bits(a), op.bits(b)) for a, b in zip(first, again))


@functools.lru_cache(maxsize=None)
def real_reference(indiv, n, q):
    import miraculix_amd as m
    snps = 40
    codes, Y, W = sr.binary_case(indiv, snps, n, q, seed=21)
    fits = [m.assoc_logistic_null(Y[:, c], W) for c in range(n)]          # the null is fitted by the library entry
    R, Wt, H = (np.asfortranarray(np.concatenate([np.reshape(getattr(f, k), (indiv, -1)) for f in fits], axis=1)) for k in ("r", "w", "H"))
    return codes, sr.pack(codes), Y, W, fits, (R, Wt, H), sr.bounded_score(codes, R, Wt, H)


@pytest.mark.parametrize("n, q", [(1, 3), (4, 10)])
@pytest.mark.parametrize("indiv", [67, 1027, 4099])
def test_real_data_within_four_times_the_forward_bound(mx, indiv, n, q):
    snps = 40
    codes, P, Y, W, fits, (R, Wt, H), (ref, bound, sww) = real_reference(indiv, n, q)
    assert 0.2 < Y.mean() < 0.6 and abs((codes < 0).mean() - 0.05) < 0.02 and H.shape[1] == n * (q + 1)
    keep = ref[1] > 1e-6 * sww
    assert keep.mean() > 0.9
    got, nobs = run(mx, P, snps, indiv, R, Wt, H)
    assert np.array_equal(nobs, (codes >= 0).sum(1))
    for name, g, r, b in zip(("score", "var", "z"), got, ref, bound):
        err = np.abs(g.astype(sr.LD) - r)[keep]
        print(f"indiv {indiv} n {n} q {q} {name}: max |err| / bound = {float((err / b[keep]).max()):.3g}")
        assert np.all(err <= 4 * b[keep]), name
    # the definition: U^2 / V of the library equals the textbook form with an explicit (C^T W C)^-1, within the same bound
    C = np.concatenate([np.ones((indiv, 1)), W], axis=1)
    for c in range(n):
        chi2 = sr.textbook_chi2(codes, Y[:, c], C, fits[c].gamma)
        u, v = got[0][:, c].astype(sr.LD), got[1][:, c].astype(sr.LD)
        b = 2 * np.abs(ref[0][:, c]) * bound[0][:, c] / ref[1][:, c] + ref[0][:, c] ** 2 / ref[1][:, c] * bound[1][:, c] / ref[1][:, c]
        k = keep[:, c]
        ratio = float((np.abs(u * u / v - chi2)[k] / b[k]).max())
        print(f"indiv {indiv} n {n} q {q} trait {c} chi2 against the textbook form: max |err| / bound = {ratio:.3g}")
        assert ratio <= 4
    # the Python entries: the same call from R, Wt, H, the whole chain from Y and the covariates, and device tensors
    res = mx.assoc_score(P, snps, indiv, R, Wt, H)
    assert all(np.array_equal(op.bits(a), op.bits(g)) for a, g in zip((res.score, res.var, res.z), got)) and np.array_equal(res.nobs, nobs)
    full = mx.assoc_logistic(P, snps, indiv, Y, covariates=W)
    assert all(np.array_equal(op.bits(a), op.bits(g)) for a, g in zip((full.score, full.var, full.z), got))
    import torch
    rt = mx.assoc_score(_dev(P), snps, indiv, *(torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (R, Wt, H)))
    assert rt.z.is_cuda and all(np.array_equal(op.bits(op.readback(a)), op.bits(g)) for a, g in zip((rt.score, rt.var, rt.z), got))


def test_the_python_entry_takes_one_dimensional_operands_and_out(mx):
    indiv, n, q = 1027, 1, 3
    codes, P, Y, W, fits, (R, Wt, H), _ = real_reference(indiv, n, q)
    a = mx.assoc_logistic(P, 40, indiv, Y[:, 0], covariates=W)
    b = mx.assoc_score(P, 40, indiv, R[:, 0], Wt[:, 0], H)
    assert a.z.shape == (40,) and b.z.shape == (40,) and np.array_equal(op.bits(a.z), op.bits(b.z)) and np.array_equal(op.bits(a.var), op.bits(b.var))
    out = {"z": np.full((40, 1), SENTINEL, order="F")}
    c = mx.assoc_score(P, 40, indiv, R, Wt, H, out=out)
    assert c.z is out["z"] and c.score is None and c.var is None and np.array_equal(op.bits(out["z"][:, 0]), op.bits(b.z))
    d = mx.assoc_score(P, 40, indiv, R, Wt)                      # no projection columns: kh = 0, V = sum w x^2
    assert np.all(d.var[:, 0] > b.var) and np.allclose(d.score[:, 0], b.score, rtol=0, atol=1e-9 * np.abs(b.score).max())          # (another column count: not the same bits)
