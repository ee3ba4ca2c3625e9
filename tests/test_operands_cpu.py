"""The operand helpers of tests/_operands.py do what the GPU tests rely on: dirty() changes the padding fields and nothing else, misaligned() lands on the
address it promises with the same bytes, and every shape of the two GPU modules has padding fields on the axis it is used for."""
import numpy as np
import pytest

import _operands as ops
from _util import make_problem, unpack_2bit


def _fields(P):
    return np.stack([(P >> (2 * q)) & 3 for q in range(4)], axis=-1).reshape(P.shape[0], -1)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 61, 67, 129, 261, 526, 1001])
@pytest.mark.parametrize("code", ops.CODES)
def test_dirty_touches_the_padding_fields_only(k, code):
    rng = np.random.default_rng(k)
    rows = 37
    P = rng.integers(0, 256, (rows, (k + 3) // 4), dtype=np.uint8)
    pad = ops.padding_fields(k)
    if pad:
        P[:, -1] &= np.uint8((1 << (2 * (4 - pad))) - 1)             # clean padding, as pack_plink leaves it
    D = ops.dirty(P, k, code)
    assert D is not P and D.dtype == np.uint8 and D.shape == P.shape
    for is_plink in (True, False):
        assert np.array_equal(unpack_2bit(D, k, is_plink), unpack_2bit(P, k, is_plink))
    assert np.array_equal(_fields(D)[:, :k], _fields(P)[:, :k])
    assert np.array_equal(D[:, :-1], P[:, :-1])
    if pad == 0:
        assert np.array_equal(D, P)
        return
    assert np.all(D[:, -1] != P[:, -1]), "every row's last byte differs"
    tail = _fields(D)[:, k:]
    assert tail.shape[1] == pad
    if code == "random":
        assert np.all(tail >= 1) and np.all(tail == tail[:, :1]) and len(np.unique(tail[:, 0])) == 3
        assert np.array_equal(D, ops.dirty(P, k, code)), "fixed seed"
    else:
        assert np.all(tail == code)
    assert np.array_equal(ops.dirty(D, k, code), D)                   # dirty padding in: the same pattern out


def test_dirty_on_generated_problems():
    for snps, indiv in ops.PADDING_OBJECT_SHAPES:
        prob = make_problem(snps, indiv, 1, seed=3, missing_frac=0.05)
        for code in ops.CODES:
            assert np.array_equal(unpack_2bit(ops.dirty(prob["plink"], indiv, code), indiv), unpack_2bit(prob["plink"], indiv))
            assert np.array_equal(unpack_2bit(ops.dirty(prob["plink_t"], snps, code), snps), unpack_2bit(prob["plink_t"], snps))


def test_every_shape_has_padding_fields_on_the_axis_it_is_used_for():
    for snps, indiv in ops.PADDING_OBJECT_SHAPES:                     # both packed matrices of an object
        assert ops.padding_fields(snps) > 0 and ops.padding_fields(indiv) > 0, (snps, indiv)
    assert {ops.padding_fields(k) for s, i in ops.PADDING_OBJECT_SHAPES for k in (s, i)} >= {1, 3}
    assert [((i + 3) // 4, (s + 3) // 4) for s, i in ops.PADDING_OBJECT_SHAPES] == [(66, 17), (132, 68)]
    assert all(p % 4 == 0 for p in ((526 + 3) // 4, (270 + 3) // 4)), "the tiled transpose runs on (270, 526)"
    for k, rows in ops.PADDING_XPROD_SHAPES:
        assert ops.padding_fields(k) > 0, k
    for snps, indiv in ops.PADDING_LD_SHAPES:                         # LD: SNP-major rows of indiv fields
        assert ops.padding_fields(indiv) > 0, (snps, indiv)
    for snps, indiv in ops.PADDING_GRM_SHAPES:                        # GRM: individual-major rows of snps fields
        assert ops.padding_fields(snps) > 0, (snps, indiv)
    # alignment: two shapes whose pitches are multiples of 4 bytes on both axes (only the base moves a row off the dword path), one ragged
    for snps, indiv in ops.ALIGNMENT_SHAPES[:2]:
        assert ((snps + 3) // 4) % 4 == 0 and ((indiv + 3) // 4) % 4 == 0
    assert ((67 + 3) // 4) % 4 and ((261 + 3) // 4) % 4


@pytest.mark.parametrize("dtype,offsets", [(np.uint8, ops.BYTE_OFFSETS), (np.int32, ops.INT_OFFSETS), (np.float64, ops.WIDE_OFFSETS), (np.int64, ops.WIDE_OFFSETS)])
def test_misaligned_host_buffers(dtype, offsets):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 200, (13, 7)).astype(dtype)
    if dtype == np.float64:
        a[3, 2] = np.nan
    for e in (0,) + tuple(offsets):
        m, addr = ops.misaligned(a, e)
        assert addr == m.ctypes.data and addr % 64 == e * a.dtype.itemsize
        assert addr % a.dtype.itemsize == 0, "never below the natural alignment"
        assert m.dtype == a.dtype and m.shape == a.shape and m.flags.c_contiguous and m.flags.writeable
        assert np.array_equal(ops.bits(m), ops.bits(a))
        before = a.copy()
        m[...] = 201                                                  # a buffer of its own
        assert np.array_equal(ops.bits(a), ops.bits(before))
    assert {o * np.dtype(dtype).itemsize % 16 for o in offsets} == {np.uint8: {1, 2, 3, 5}, np.int32: {4, 8, 12}, np.float64: {8}, np.int64: {8}}[dtype]


def test_misaligned_torch_buffers():
    """the torch path of misaligned(), on the host: the tensor the GPU tests hand over as a device operand"""
    torch = pytest.importorskip("torch")
    for dtype, offsets in ((np.uint8, ops.BYTE_OFFSETS), (np.int32, ops.INT_OFFSETS), (np.float64, ops.WIDE_OFFSETS), (np.int64, ops.WIDE_OFFSETS)):
        a = np.random.default_rng(6).integers(0, 200, (5, 9)).astype(dtype)
        for e in (0,) + tuple(offsets):
            t, addr = ops.misaligned(a, e, device="cpu")
            assert isinstance(t, torch.Tensor) and addr == t.data_ptr() and addr % 64 == e * a.dtype.itemsize
            assert tuple(t.shape) == a.shape and t.is_contiguous() and np.array_equal(ops.readback(t), a)
