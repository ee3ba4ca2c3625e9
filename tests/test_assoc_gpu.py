"""mxa_assoc_linear on the device.  The exact family (tests/_assoc_ref.py: every sum the definition names is exact in fp64, the residualization is the identity)
bit for bit against the documented chain, NaN positions included, over the shapes at which the scan and the product change path; real data against the
long-double reference within 4 x its first-order forward bound; run-to-run identity; and the process-wide centring option, which the call neither obeys nor
changes.

Shapes: indiv in {19, 67, 259, 1027} (partial last bytes; the 16-byte word and the 128-genotype slab edges), snps in {1, 255, 257, 700} (tile-row edges of the
product), (n, k) in {(1, 0), (1, 2), (3, 4), (2, 15), (17, 16)} (the product's n <= 6 and n >= 7 routes, a 4q + r peel, the scan's 16-column chunk).  indiv = 19
has 15 non-constant Walsh functions only: the family needs k of them for Q and one more for Y, so (2, 15) and (17, 16) do not exist there.  Long rows,
indiv in {16387, 65539} (257 and 1025 words of 64 genotypes: a thread's second word in flight, and a second round of its loop), run with a few SNPs."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import _assoc_ref as ar
import _operands as op

pytestmark = pytest.mark.gpu

INDIV = (19, 67, 259, 1027)
SNPS = (1, 255, 257, 700)
NK = ((1, 0), (1, 2), (3, 4), (2, 15), (17, 16))
SENTINEL = -7.5


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


@functools.lru_cache(maxsize=None)
def exact_case(indiv, snps, n, k, missing=0.05):
    """(codes, packed rows, Y, Q, (beta, se, t, nobs) of the chain): computed once, shared, read-only"""
    Y, Q = ar.exact_family(indiv, n, k, seed=17)
    codes = ar.genotypes(snps, indiv, seed=29, missing=missing, special=missing > 0)
    out = (codes, ar.pack(codes), Y, Q, ar.chain_exact(codes, Y, Q))
    for a in out[:4] + out[4]:
        a.setflags(write=False)
    return out


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")          # (a copy: the shared cases are read-only)


def _columns(M, ld, device, fill=np.nan):
    """the column-major operand of M (rows, cols) with leading dimension ld (the rows behind a column hold `fill`), on the host or the device"""
    rows, cols = M.shape
    buf = np.full((max(cols, 1), ld), fill)
    buf[:cols, :rows] = M.T
    return _dev(buf) if device else buf


def run(mx, plink, snps, indiv, Y, Q, dev=(False, False, False, False), ldy=None, ldq=None, ldo=None, want=(True, True, True), nobs_dev=False, operands=None):
    """one call through the C ABI; dev: plink, Y, Q, results on the device.  Returns (beta, se, t) as (snps, n) arrays (None where not wanted), nobs, dof, after
    checking that nothing beyond row snps - 1 of a column or beyond column n - 1 was written."""
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    n, k = Y.shape[1], Q.shape[1]
    ldy, ldq, ldo = ldy or indiv, ldq or indiv, ldo or snps
    if operands is None:
        operands = (_dev(plink) if dev[0] else np.ascontiguousarray(plink), _columns(Y, ldy, dev[1]), _columns(Q, ldq, dev[2]) if k else None)
    P, yb, qb = operands
    res = [(_dev(np.full((n + 1, ldo), SENTINEL)) if dev[3] else np.full((n + 1, ldo), SENTINEL)) if w else None for w in want]
    nobs = _dev(np.full(snps + 1, -3, np.int32)) if nobs_dev else np.full(snps + 1, -3, np.int32)
    dof = ctypes.c_int(-3)
    rc = L.mxa_assoc_linear(p(P), snps, indiv, p(yb), ldy, n, p(qb), ldq, k, p(res[0]), p(res[1]), p(res[2]), ldo, p(nobs), ctypes.byref(dof))
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
    return outs, nobs[:snps], dof.value


def check_exact(got, nobs, dof, case, indiv, k):
    want = case[4]
    for name, g, w in zip(("beta", "se", "t"), got, want[:3]):
        if g is not None:
            assert ar.same_bits(g, w), (name, np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))[:5])
    assert np.array_equal(nobs, want[3]) and dof == indiv - k - 2


MEMBERS = [(i, n, k) for i in INDIV for n, k in NK if k <= i - 5]          # indiv = 19: the family has no member with k = 15 or 16 (module docstring)


@pytest.mark.parametrize("snps", SNPS)
@pytest.mark.parametrize("indiv, n, k", MEMBERS)
def test_exact_family_bit_for_bit(mx, indiv, snps, n, k):
    case = exact_case(indiv, snps, n, k)
    codes, P, Y, Q, _ = case
    if snps == 1:       # an ordinary row with missing calls: the one SNP compares finite bits
        assert 0 < (codes[0] < 0).sum() < indiv and np.all(np.isfinite(case[4][2]))
    if snps >= 7:       # the patterns are there: N = 0, one called individual, constant on the called, a missing code in the last field, no missing code
        assert np.all(codes[0] < 0) and (codes[1] >= 0).sum() == 1 and codes[4, -1] < 0 and not np.any(codes[5] < 0) and np.any(codes[6:] < 0)
    got, nobs, dof = run(mx, P, snps, indiv, Y, Q)
    check_exact(got, nobs, dof, case, indiv, k)
    if snps >= 7:
        assert not np.any(np.isfinite(got[2][:4])) and np.isfinite(got[2][4:]).mean() > 0.9          # the four uninformative rows, and hardly another one


@pytest.mark.parametrize("n, k", [(3, 4), (17, 16)])
@pytest.mark.parametrize("indiv", [16387, 65539])
def test_exact_family_long_rows_bit_for_bit(mx, indiv, n, k):
    """rows of more than 256 and more than 512 words: every thread of the scan takes a second word in flight, and at 65539 a second round of its loop.  Nine
    SNPs (the six edge patterns and three ordinary rows with 5 % missing calls); host and device pointers; the 4097- and 16385-byte rows start at every
    offset of a 16-byte word, and once more from a base one byte off a 64-byte boundary"""
    snps = 9
    case = exact_case(indiv, snps, n, k)
    assert (indiv + 3) // 4 > 256 * 16 and np.any(case[0][6:] < 0) and np.all(np.isfinite(case[4][2][6:]))
    for dev in (False, True):
        got, nobs, dof = run(mx, case[1], snps, indiv, case[2], case[3], dev=(dev,) * 4)
        check_exact(got, nobs, dof, case, indiv, k)
        P, _ = op.misaligned(case[1], 1, dev)
        yb, qb = _columns(case[2], indiv, dev), _columns(case[3], indiv, dev)
        got, nobs, dof = run(mx, None, snps, indiv, case[2], case[3], operands=(P, yb, qb))
        check_exact(got, nobs, dof, case, indiv, k)


@pytest.mark.parametrize("indiv, n, k", MEMBERS)
def test_exact_family_without_any_missing_code(mx, indiv, n, k):
    """no 01 field anywhere: M is zero and the scan skips its further column chunks"""
    case = exact_case(indiv, 257, n, k, missing=0.0)
    assert not np.any(case[0] < 0)
    got, nobs, dof = run(mx, case[1], 257, indiv, case[2], case[3], dev=(True, False, False, True))
    check_exact(got, nobs, dof, case, indiv, k)
    assert np.all(nobs == indiv)


def test_host_and_device_pointers_in_every_combination(mx):
    indiv, snps, n, k = 67, 257, 3, 4
    case = exact_case(indiv, snps, n, k)
    for dev in itertools.product((False, True), repeat=4):
        got, nobs, dof = run(mx, case[1], snps, indiv, case[2], case[3], dev=dev, nobs_dev=dev[0])
        check_exact(got, nobs, dof, case, indiv, k)
    # mixed host and device result pointers are refused, nothing is written
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    h, d = np.full((n, snps), SENTINEL), _dev(np.full((n, snps), SENTINEL))
    rc = L.mxa_assoc_linear(p(np.ascontiguousarray(case[1])), snps, indiv, p(_columns(case[2], indiv, False)), indiv, n, p(_columns(case[3], indiv, False)), indiv, k,
                            p(h), p(d), None, snps, None, None)
    assert rc == 1 and L.mxa_last_error() == 1 and np.all(h == SENTINEL) and np.all(op.readback(d) == SENTINEL)


@pytest.mark.parametrize("dev", [False, True])
def test_leading_dimensions_larger_than_needed_and_optional_outputs(mx, dev):
    indiv, snps, n, k = 259, 255, 2, 15
    case = exact_case(indiv, snps, n, k)
    got, nobs, dof = run(mx, case[1], snps, indiv, case[2], case[3], dev=(dev,) * 4, ldy=indiv + 3, ldq=indiv + 1, ldo=snps + 5)
    check_exact(got, nobs, dof, case, indiv, k)
    for want in ((False, True, True), (True, False, True), (True, True, False), (False, False, True)):
        got, nobs, dof = run(mx, case[1], snps, indiv, case[2], case[3], dev=(dev,) * 4, want=want, ldo=snps + 1)
        assert [g is not None for g in got] == list(want)
        check_exact(got, nobs, dof, case, indiv, k)
    # nobs and dof are optional too
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    b = np.full((n, snps), SENTINEL)
    assert L.mxa_assoc_linear(p(np.ascontiguousarray(case[1])), snps, indiv, p(_columns(case[2], indiv, False)), indiv, n, p(_columns(case[3], indiv, False)), indiv, k,
                              p(b), None, None, snps, None, None) == 0
    assert ar.same_bits(b.T, case[4][0])


@pytest.mark.parametrize("indiv", [19, 67, 259, 1027])
def test_dirty_padding_fields_give_the_same_bits(mx, indiv):
    snps, n, k = 257, 3, 4
    case = exact_case(indiv, snps, n, k)
    assert op.padding_fields(indiv) > 0
    for code in op.CODES:
        for dev in (False, True):
            got, nobs, dof = run(mx, op.dirty(case[1], indiv, code), snps, indiv, case[2], case[3], dev=(dev, False, False, False))
            check_exact(got, nobs, dof, case, indiv, k)


@pytest.mark.parametrize("device", [False, True])
def test_pointers_off_a_64_byte_boundary_give_the_same_bits(mx, device):
    indiv, snps, n, k = 259, 257, 3, 4          # 65-byte rows: at an aligned base every 16th row takes the 16-byte loads, the others the byte loads; off it, all do
    case = exact_case(indiv, snps, n, k)
    yb, qb = _columns(case[2], indiv, False), _columns(case[3], indiv, False)
    for off in op.BYTE_OFFSETS:
        P, _ = op.misaligned(case[1], off, device)
        got, nobs, dof = run(mx, None, snps, indiv, case[2], case[3], operands=(P, _dev(yb) if device else yb, _dev(qb) if device else qb))
        check_exact(got, nobs, dof, case, indiv, k)
    for off in op.WIDE_OFFSETS:
        ym, _ = op.misaligned(yb, off, device)
        qm, _ = op.misaligned(qb, off, device)
        got, nobs, dof = run(mx, None, snps, indiv, case[2], case[3], operands=(_dev(case[1]) if device else np.ascontiguousarray(case[1]), ym, qm))
        check_exact(got, nobs, dof, case, indiv, k)


def test_a_small_staging_chunk_gives_the_same_bits(mx, monkeypatch):
    """MXA_ASSOC_CHUNK_ROWS: a host matrix staged in chunks of 37 rows (19 chunks, the last one partial), and one row at a time"""
    indiv, snps = 1027, 700
    for n, k, rows in ((17, 16, "37"), (3, 4, "1"), (3, 4, "100000")):
        case = exact_case(indiv, snps, n, k)
        monkeypatch.setenv("MXA_ASSOC_CHUNK_ROWS", rows)
        got, nobs, dof = run(mx, case[1], snps, indiv, case[2], case[3])
        check_exact(got, nobs, dof, case, indiv, k)
    monkeypatch.delenv("MXA_ASSOC_CHUNK_ROWS")


@functools.lru_cache(maxsize=None)
def real_reference(indiv, n, k):
    import miraculix_amd as m
    codes, Y, W = ar.real_case(indiv, 513, n, k, seed=21)
    Q = m.assoc_basis(W)
    return codes, ar.pack(codes), Y, Q, ar.bounded(codes, Y, Q)


@pytest.mark.parametrize("n, k", [(1, 3), (8, 10)])
@pytest.mark.parametrize("indiv", [67, 1027, 4099])
def test_real_data_within_four_times_the_forward_bound(mx, indiv, n, k):
    snps = 513
    codes, P, Y, Q, (ref, bound, sxx, v0) = real_reference(indiv, n, k)
    assert abs(Y.mean() - 100) < 5 and max(abs(np.corrcoef(Y[:, 0], Q[:, j])[0, 1]) for j in range(k)) > 0.1 and abs((codes < 0).mean() - 0.05) < 0.01
    keep = sxx >= 1e-6 * v0
    assert np.all(keep)                       # the data leave out no SNP
    got, nobs, dof = run(mx, P, snps, indiv, Y, Q)
    assert np.array_equal(nobs, (codes >= 0).sum(1)) and dof == indiv - k - 2
    for name, g, r, b in zip(("beta", "se", "t"), got, ref, bound):
        ok, ratio = ar.within_bound(g, r, b, keep)
        print(f"indiv {indiv} n {n} k {k} {name}: max |err| / bound = {ratio:.3g}")
        assert ok, (name, ratio)
    # the Python entry: the same call, raw covariates or the basis, host or device tensors
    res = mx.assoc_linear(P, snps, indiv, Y, Q=Q)
    assert all(np.array_equal(op.bits(a), op.bits(g)) for a, g in zip((res.beta, res.se, res.t), got)) and np.array_equal(res.nobs, nobs) and res.dof == dof
    import torch
    rt = mx.assoc_linear(_dev(P), snps, indiv, torch.from_numpy(Y).to("cuda:0"), Q=torch.from_numpy(Q).to("cuda:0"))
    assert rt.t.is_cuda and all(np.array_equal(op.bits(op.readback(a)), op.bits(g)) for a, g in zip((rt.beta, rt.se, rt.t), got))


def test_the_python_entry_takes_raw_covariates_one_dimensional_y_and_out(mx):
    indiv, n, k = 1027, 1, 3
    codes, P, Y, Q, _ = real_reference(indiv, n, k)
    _, _, W = ar.real_case(indiv, 513, n, k, seed=21)
    a = mx.assoc_linear(P, 513, indiv, Y[:, 0], covariates=W)
    b = mx.assoc_linear(P, 513, indiv, Y, Q=Q)
    assert a.t.shape == (513,) and np.array_equal(op.bits(a.t), op.bits(b.t[:, 0])) and np.array_equal(op.bits(a.beta), op.bits(b.beta[:, 0]))
    out = {"t": np.full((513, 1), SENTINEL, order="F")}
    c = mx.assoc_linear(P, 513, indiv, Y, Q=Q, out=out)
    assert c.t is out["t"] and c.beta is None and c.se is None and np.array_equal(op.bits(out["t"]), op.bits(b.t))
    d = mx.assoc_linear(P, 513, indiv, Y)                      # no covariates: k = 0
    assert d.dof == indiv - 2 and np.all(np.isfinite(d.t))


def test_run_to_run_and_the_centring_option(mx):
    """two calls give the same bits; setOptions_compressed with centring on changes nothing, and the process-wide option is what it was: a centred product before
    and after the call gives the same bits, those of the centred oracle.  The scan's one-shot object carries no allele frequencies, and a centred product on
    such an object is refused (error 6): with centring on, the calls below succeed only because the thread-local override makes their products uncentred.
    The test ends with centring on, the library's state before any setOptions_compressed call."""
    from _util import Oracle, make_B, make_problem
    indiv, n, k = 1027, 8, 10
    codes, P, Y, Q, _ = real_reference(indiv, n, k)
    dg = mx.dgemm_compressed
    dg.set_options(use_gpu=True, not_center=True, verbose=0)
    first, nobs, _ = run(mx, P, 513, indiv, Y, Q)
    dg.set_options(use_gpu=True, not_center=False, verbose=0)
    prob = make_problem(300, 200, 4, seed=5)
    obj = dg.init_compressed(prob["plink"], prob["plink_t"], prob["snps"], prob["indiv"], prob["f"], 4)
    B = make_B(prob["indiv"], 4, seed=6)
    Bf = np.asfortranarray(B[:, :prob["indiv"]].T)
    C1 = np.array(dg.dgemm_compressed_main(True, obj, Bf, prob["snps"], prob["indiv"]), copy=True)
    for _ in range(2):
        again, nobs2, _ = run(mx, P, 513, indiv, Y, Q, dev=(True, True, True, True))
        assert all(np.array_equal(op.bits(a), op.bits(b)) for a, b in zip(first, again)) and np.array_equal(nobs, nobs2)
    C2 = np.array(dg.dgemm_compressed_main(True, obj, Bf, prob["snps"], prob["indiv"]), copy=True)
    dg.free_compressed(obj)
    assert np.array_equal(op.bits(C1), op.bits(C2))
    centred, plain = (Oracle().dgemm_dense(1, prob, B, c)[:, :prob["snps"]] for c in (1, 0))
    assert np.abs(C2.T - centred).max() <= 1e-11 * np.abs(centred).max() < np.abs(C2.T - plain).max()
