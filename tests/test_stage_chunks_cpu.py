"""The .bed entries' checks of the file and of the range, which bed_range_to_handle (mxa_stage.cpp) makes before it selects a device -- so they run
without one, like test_abi_cpu.py::test_bed_reader_rejects_bad_magic -- and MXA_STAGE_CHUNK_ROWS in the documents.  Each refusal returns 1, leaves
*compressed NULL and names the problem in mxa_last_error_string()."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNPS, INDIV = 700, 1027
BPS = (INDIV + 3) // 4
BED_MAGIC = bytes([0x6C, 0x1B, 0x01])


@pytest.fixture(scope="module")
def L():
    import miraculix_amd as m
    return m.load_shared_library()


def _bed(tmp_path, payload_bytes):
    p = tmp_path / "x.bed"
    p.write_bytes(BED_MAGIC + bytes(payload_bytes))
    return str(p).encode()


def _refused(L, rc, obj):
    assert rc == 1 and not obj.value
    assert L.mxa_last_error() != 0
    return (L.mxa_last_error_string() or b"").decode()


@pytest.mark.parametrize("delta", [-1, 1])
def test_bed_file_one_byte_too_short_or_too_long(L, tmp_path, delta):
    want = 3 + SNPS * BPS
    path = _bed(tmp_path, SNPS * BPS + delta)
    for call in ("whole", "range"):
        obj = ctypes.c_void_p(12345)
        if call == "whole":
            rc = L.mxa_bed2compressed(path, SNPS, INDIV, 1, ctypes.byref(obj), None, None, None)
        else:
            rc = L.mxa_bed2compressed_range(path, SNPS, INDIV, 5, 262, 1, ctypes.byref(obj), None)
        msg = _refused(L, rc, obj)
        assert f"has {want + delta} bytes" in msg and f"= {want}" in msg and f"ceil({INDIV}/4)" in msg, msg


def test_bed_path_that_does_not_exist(L, tmp_path):
    path = str(tmp_path / "nothing_here.bed").encode()
    for call in ("whole", "range"):
        obj = ctypes.c_void_p(12345)
        if call == "whole":
            rc = L.mxa_bed2compressed(path, SNPS, INDIV, 1, ctypes.byref(obj), None, None, None)
        else:
            rc = L.mxa_bed2compressed_range(path, SNPS, INDIV, 0, 1, 1, ctypes.byref(obj), None)
        msg = _refused(L, rc, obj)
        assert "cannot open" in msg and "nothing_here.bed" in msg, msg


@pytest.mark.parametrize("begin,end", [(5, 5), (262, 5), (-1, 4), (0, SNPS + 1), (SNPS, SNPS + 1)])
def test_bed_range_outside_the_file(L, tmp_path, begin, end):
    """snp_begin == snp_end, snp_begin < 0, snp_end > snps: refused on the arguments alone (the file is well formed)"""
    path = _bed(tmp_path, SNPS * BPS)
    obj = ctypes.c_void_p(12345)
    msg = _refused(L, L.mxa_bed2compressed_range(path, SNPS, INDIV, begin, end, 1, ctypes.byref(obj), None), obj)
    assert f"[{begin}, {end}) of {SNPS}" in msg and "snp_begin < snp_end <= snps" in msg, msg


def test_the_knob_is_documented_where_its_neighbours_are():
    def read(*parts):
        return open(os.path.join(ROOT, *parts)).read()

    header = read("include", "miraculix_amd.h")
    for entry in (r"void plink2compressed\(", r"int mxa_bed2compressed\(", r"int snp_multiply_gpu\("):
        comment = re.search(r"/\*((?:(?!\*/).)*)\*/\s*" + entry, header, flags=re.S).group(1)
        for phrase in ("MXA_STAGE_CHUNK_ROWS", "read per call", "bit-identical for every chunk size"):
            assert phrase in comment, (entry, phrase)
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = read(doc)
        at = text.index("MXA_STAGE_CHUNK_ROWS")
        assert "bit-identical for every chunk size" in " ".join(text[at: at + 900].split()), doc
    design = read("DESIGN.md")
    assert design.index("### 3.5 ") < design.index("MXA_STAGE_CHUNK_ROWS") < design.index("### 3.6 ")
    internal = read("miraculix_amd", "csrc", "mxa_internal.h")
    body = internal[internal.index("inline long stage_chunk_rows("):]
    body = body[: body.index("\n}") + 2]
    assert 'getenv("MXA_STAGE_CHUNK_ROWS")' in body and "static" not in body          # read per call, nothing cached
    users = {"mxa_stage.cpp": 2, "mxa_crossprod.hip": 2, "mxa_ldwindow.hip": 1}        # the three loops and the two pre-flights
    for name, count in users.items():
        assert read("miraculix_amd", "csrc", name).count("stage_chunk_rows(") == count, name
