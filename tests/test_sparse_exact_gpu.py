"""sparse_times_plink on the device, bit for bit against the documented chain (tests/_sparse_ref.py; held to the long-double oracle and to the reference
library's outputs, and shown to discriminate, in tests/test_sparse_exact_cpu.py).  Every call goes through the raw C ABI with a sentinel-filled C of
Ldc x (entries + 1): the whole Ldc x entries block must equal the chain -- zeros in rows nIdx .. Ldc - 1 included -- and the column behind it must keep the
sentinel.

Sizes (_sparse_ref.ENTRIES / NIDX / ROWS): entries around the packed byte (1 .. 9), around the 512-entry workgroup (511 .. 513) and two workgroups (1023,
1029); an odd byte count (1, 3, 4, 9, 513) has the lane that holds one byte only; nIdx around the 16-row workgroup; 1, 37 and 300 packed rows.  The slabs of a
host C and the bounce chunks of a host packed matrix are reached through MXA_SPARSE_SLAB_BYTES / MXA_SPARSE_CHUNK_BYTES; that a call ran in the pieces a test
means is read from the line the driver prints about them under PRINT_LEVEL=1."""
import itertools
import re

import numpy as np
import pytest

import _operands as op
import _sparse_ref as sr

pytestmark = pytest.mark.gpu

SENTINEL = -7.5
HOST, DEVICE = (False,) * 5, (True,) * 5


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")          # (a copy: the shared cases are read-only)


def call(mx, c, trans=False, ldc=None, dev=HOST, ia=None, ja=None, a=None, P="case", nidx=None, null=()):
    """one call through the C ABI.  dev: packed matrix, rowIdxB, colIdxB, B, C on the device.  Returns (status, the Ldc x entries block as (entries, Ldc),
    the whole buffer read back)."""
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    ia, ja, a = (c.ia if ia is None else ia), (c.ja if ja is None else ja), (c.a if a is None else a)
    nidx = len(ia) - 1 if nidx is None else nidx
    ldc = nidx if ldc is None else ldc
    put = lambda x, d: _dev(x) if d else np.array(x, order="C")
    Pb = put(c.P, dev[0]) if isinstance(P, str) else P
    ib, jb, ab = put(ia, dev[1]), put(ja, dev[2]), put(a, dev[3])
    buf = put(np.full((c.entries + 1, max(ldc, 1)), SENTINEL), dev[4])
    snps, indiv = (c.entries, c.rows) if trans else (c.rows, c.entries)
    L.sparse_times_plink(b"N", b"T" if trans else b"N", None if trans else p(Pb), p(Pb) if trans else None, snps, indiv, nidx,
                         None if "ia" in null else p(ib), None if "ja" in null else p(jb), None if "a" in null else p(ab), p(buf), ldc)
    out = op.readback(buf)
    return L.mxa_last_error(), out[:c.entries, :ldc], out


def check(mx, c, trans=False, ldc=None, dev=HOST, **kw):
    """the call succeeds, writes the chain's bits over Ldc x entries and nothing behind them"""
    status, C, out = call(mx, c, trans=trans, ldc=ldc, dev=dev, **kw)
    assert status == 0, mx.lib.last_error()
    want = c.want(ldc)
    assert C.shape == want.shape
    assert sr.same_bits(C, want), (trans, ldc, dev, np.argwhere(~((C == want) | (np.isnan(C) & np.isnan(want))))[:5])
    assert np.all(out[c.entries] == SENTINEL)
    return C


def pieces(capfd):
    """what the calls since the last look said about their staging: ([bounce chunks of each host matrix upload], [slabs of each host C])"""
    out = capfd.readouterr().out
    return [int(n) for n in re.findall(r"uploaded in (\d+) chunk", out)], [int(n) for n in re.findall(r"host C in (\d+) slab", out)]


@pytest.mark.parametrize("rows", sr.ROWS)
@pytest.mark.parametrize("nidx", sr.NIDX)
@pytest.mark.parametrize("entries", sr.ENTRIES)
def test_tile_edges_bit_for_bit(mx, entries, nidx, rows):
    """both orientations ('N': rows = snps, reads plink; 'T': rows = indiv, reads plink_transposed), Ldc = nIdx and nIdx + 3, every operand on the host and
    every operand on the device: Ldc > nIdx on a device C, unsorted and duplicate columns on the host-gather path and on the in-place device path, the
    one-byte lane at entries 1, 3, 4, 9 and 513"""
    c = sr.tile_case(entries, nidx, rows)
    for trans, extra, dev in itertools.product((False, True), (0, 3), (HOST, DEVICE)):
        check(mx, c, trans=trans, ldc=nidx + extra, dev=dev)


def test_pointer_kinds_in_every_combination_and_run_to_run(mx):
    """packed matrix, CSR arrays and C each on the host or the device (eight combinations), then row pointers on the host with columns and values on the
    device; every call gives the chain's bits, so host and device, and two identical calls, give identical bits"""
    c = sr.tile_case(513, 17, 37)
    for dP, dS, dC in itertools.product((False, True), repeat=3):
        first = check(mx, c, ldc=20, dev=(dP, dS, dS, dS, dC))
        again = check(mx, c, ldc=20, dev=(dP, dS, dS, dS, dC))
        assert np.array_equal(op.bits(first), op.bits(again))
    for dP, dC in itertools.product((False, True), repeat=2):
        check(mx, c, ldc=20, dev=(dP, False, True, True, dC))
        check(mx, c, trans=True, dev=(dP, True, False, True, dC))


def test_host_c_in_three_slabs(mx, monkeypatch, capfd):
    """entries = 1029, nIdx = 17, Ldc = 19 with a device buffer of 512 columns: slabs of 512, 512 and 5 columns, e_base = 0, 512, 1024"""
    entries, nidx, rows = sr.SLAB_CASE
    c, ldc = sr.tile_case(entries, nidx, rows), nidx + 2
    assert entries == 2 * 512 + 5 and ldc == 19
    monkeypatch.setenv("PRINT_LEVEL", "1")
    whole = check(mx, c, ldc=ldc)
    assert pieces(capfd) == ([1], [1])
    monkeypatch.setenv("MXA_SPARSE_SLAB_BYTES", str(8 * ldc * 512))
    for trans, dP in itertools.product((False, True), repeat=2):
        sliced = check(mx, c, trans=trans, ldc=ldc, dev=(dP, False, False, False, False))
        assert np.array_equal(op.bits(sliced), op.bits(whole))
        assert pieces(capfd) == ([] if dP else [1], [3])
    monkeypatch.setenv("MXA_SPARSE_SLAB_BYTES", "1")                         # no slab is narrower than 512 columns
    check(mx, c, ldc=ldc)
    assert pieces(capfd)[1] == [3]
    monkeypatch.setenv("MXA_SPARSE_SLAB_BYTES", str(8 * ldc * 1024))         # 1024 and 5
    check(mx, c, ldc=ldc)
    assert pieces(capfd)[1] == [2]
    monkeypatch.delenv("MXA_SPARSE_SLAB_BYTES")
    monkeypatch.delenv("PRINT_LEVEL")


def test_host_matrix_in_several_bounce_chunks(mx, monkeypatch, capfd):
    """a host packed matrix of 300 rows of 129 bytes, of which S refers to a part: uploaded in chunks of 7 rows (the last one partial), of one row, and
    with both knobs at once"""
    c = sr.tile_case(513, 33, 300)
    used, pitch = len(np.unique(c.ja)), (c.entries + 3) // 4
    assert used > 3 * 7 and used % 7 != 0 and used < c.rows
    monkeypatch.setenv("PRINT_LEVEL", "1")
    whole = check(mx, c, ldc=36)
    assert pieces(capfd) == ([1], [1])
    for chunk, n in ((7 * pitch, (used + 6) // 7), (1, used), (7 * pitch + 5, (used + 6) // 7)):
        monkeypatch.setenv("MXA_SPARSE_CHUNK_BYTES", str(chunk))
        for dC in (False, True):
            C = check(mx, c, ldc=36, dev=(False, False, False, False, dC))
            assert np.array_equal(op.bits(C), op.bits(whole))
            assert pieces(capfd) == ([n], [] if dC else [1])
    monkeypatch.setenv("MXA_SPARSE_SLAB_BYTES", "1")
    check(mx, c, ldc=36)
    check(mx, c, trans=True, ldc=36)
    assert pieces(capfd) == ([(used + 6) // 7] * 2, [2, 2])
    monkeypatch.delenv("MXA_SPARSE_CHUNK_BYTES")
    monkeypatch.delenv("MXA_SPARSE_SLAB_BYTES")
    monkeypatch.delenv("PRINT_LEVEL")


@pytest.mark.parametrize("name", sr.SHAPES)
def test_csr_shapes_of_their_own(mx, name):
    """all rows empty; one row of 1200 entries with duplicates; rows on packed row 0 alone, on the last packed row alone"""
    c = sr.shape_case(name)
    for trans, dev in itertools.product((False, True), (HOST, DEVICE)):
        check(mx, c, trans=trans, ldc=c.nidx + 3, dev=dev)


def test_inf_and_nan_values(mx):
    """+inf in one row, NaN in another: NaN where the chain has NaN (inf * 0 included), the same bits everywhere else"""
    c = sr.nonfinite_case()
    for dev in (HOST, DEVICE):
        C = check(mx, c, ldc=c.nidx + 3, dev=dev)
        assert np.all(np.isnan(C[:, 4])) and np.any(np.isinf(C[:, 0])) and np.any(np.isnan(C[:, 0]))


@pytest.mark.parametrize("dev", [HOST, DEVICE], ids=["host", "device"])
def test_no_sparse_row_zero_fills_ldc_by_entries(mx, dev):
    """nIdx = 0 with Ldc = 3: C is zero over 3 x entries, as the header says and the reference does"""
    c = sr.tile_case(513, 17, 37)
    for trans in (False, True):
        status, C, out = call(mx, c, trans=trans, ldc=3, dev=dev, ia=np.zeros(1, np.int32), ja=np.zeros(0, np.int32), a=np.zeros(0))
        assert status == 0, mx.lib.last_error()
        assert C.shape == (513, 3) and np.array_equal(op.bits(C), np.zeros((513, 3), np.uint64)) and np.all(out[513] == SENTINEL)


@pytest.mark.parametrize("dev", [HOST, DEVICE], ids=["host", "device"])
def test_more_sparse_rows_than_one_launch_has_row_blocks(mx, dev):
    """nIdx = 16 * 65535 + 17 (65537 row blocks: a second piece of gridDim.y), entries = 5, Ldc = nIdx + 3; non-empty rows at 16 * 65535 - 1, 16 * 65535,
    16 * 65535 + 1 and the last row"""
    c = sr.big_case()
    C = check(mx, c, ldc=c.nidx + 3, dev=dev)
    assert all(np.any(C[:, j] != 0.0) for j in (16 * 65535 - 1, 16 * 65535, 16 * 65535 + 1, c.nidx - 1))


def test_errors_leave_c_untouched_and_a_good_call_clears_the_status(mx):
    c = sr.tile_case(513, 17, 37)
    bad_first, decreasing, negative, beyond = c.ia.copy(), c.ia.copy(), c.ja.copy(), c.ja.copy()
    bad_first[0] = 1
    decreasing[3] = decreasing[2] - 1
    negative[5] = -1
    beyond[len(beyond) - 1] = c.rows
    cases = [("rowIdxB[0] != 0", dict(ia=bad_first), 1), ("decreasing row pointer", dict(ia=decreasing), 1), ("negative column", dict(ja=negative), 1),
             ("column == rows", dict(ja=beyond), 1), ("Ldc < nIdx", dict(ldc=c.nidx - 1), 7), ("NULL packed matrix", dict(P=None), 1),
             ("NULL colIdxB", dict(null=("ja",)), 1)]
    for what, kw, code in cases:
        for dev in (HOST, DEVICE):
            for trans in (False, True):
                status, _, out = call(mx, c, trans=trans, dev=dev, **kw)
                assert status == code, (what, dev, trans, status, mx.lib.last_error())
                assert np.all(out == SENTINEL), (what, dev, trans)
        check(mx, c)                                                           # a successful call clears the status
        assert mx.lib.check_library_handle().mxa_last_error() == 0
