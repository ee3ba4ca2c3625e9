"""Operand layouts of the C ABI that no generator of the suite produces: packed rows whose padding fields are not zero, and buffers whose address is not
the base of an allocation.  Plain numpy (torch only for device buffers); nothing of the library is imported.

dirty(P, k, code)             packed rows P (k fields per row, 4 per byte, low bits first): a copy in which every field at and beyond k of each row's last byte
                              holds `code` (1 = 01, the missing code; 2 = 10; 3 = 11) or, for "random", a per-row pick of 1 / 2 / 3 from a fixed seed.
misaligned(a, elems, device)  the values of `a` in a buffer that starts `elems` elements behind a 64-byte boundary; never below the natural alignment of
                              the element type (the offset is counted in elements).  Returns (array or tensor, address).
"""
import numpy as np

CODES = (1, 2, 3, "random")            # the four dirty padding patterns
BYTE_OFFSETS = (1, 2, 3, 5)            # packed bytes and keep[]
INT_OFFSETS = (1, 2, 3)                # int32: 4, 8, 12 mod 16
WIDE_OFFSETS = (1,)                    # double / long: 8 mod 16
_SEED = 20240611


def padding_fields(k):
    """number of fields at and beyond k in the last byte of a row of k fields"""
    return (-k) % 4


def dirty(P, k, code):
    P = np.ascontiguousarray(P, dtype=np.uint8)
    assert P.ndim == 2 and P.shape[1] == (k + 3) // 4, (P.shape, k)
    assert code in CODES, code
    out = P.copy()
    pad = padding_fields(k)
    if pad == 0:
        return out
    rows = P.shape[0]
    if code == "random":
        c = np.random.default_rng([_SEED, rows, k]).integers(1, 4, size=rows).astype(np.uint8)
    else:
        c = np.full(rows, code, np.uint8)
    fill = np.zeros(rows, np.uint8)
    for q in range(4 - pad, 4):
        fill |= c << np.uint8(2 * q)
    low = np.uint8((1 << (2 * (4 - pad))) - 1)                       # the fields below k of the last byte
    out[:, -1] = (out[:, -1] & low) | fill
    return out


def misaligned(a, elems, device=False):
    """(copy of `a` at `elems` elements past a 64-byte boundary, its address); device True: a torch tensor on cuda:0 (a torch device or its name: there),
    else numpy"""
    a = np.ascontiguousarray(a)
    size = a.dtype.itemsize
    assert elems >= 0 and elems * size < 64
    if device:
        import torch
        raw = torch.empty(a.nbytes + 128, dtype=torch.uint8, device=torch.device("cuda", 0) if device is True else torch.device(device))
        start = (-raw.data_ptr()) % 64 + elems * size
        view = raw[start: start + a.nbytes]
        view.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)).to(raw.device))
        out = view.view(getattr(torch, str(a.dtype))).reshape(a.shape) if a.dtype != np.uint8 else view.reshape(a.shape)
        addr = out.data_ptr()
        assert addr % 64 == elems * size, (addr % 64, elems, size)
        assert np.array_equal(out.cpu().numpy().view(np.uint8).reshape(-1), a.reshape(-1).view(np.uint8))
        return out, addr
    raw = np.empty(a.nbytes + 128, np.uint8)
    start = (-raw.ctypes.data) % 64 + elems * size
    out = raw[start: start + a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    addr = out.ctypes.data
    assert addr % 64 == elems * size, (addr % 64, elems, size)
    assert np.array_equal(out.reshape(-1).view(np.uint8), a.reshape(-1).view(np.uint8))      # the bytes (NaN payloads included)
    return out, addr


def readback(x):
    """numpy copy of a numpy array or a torch tensor"""
    return x.detach().cpu().numpy().copy() if hasattr(x, "detach") else np.array(x, copy=True)


# ---- the shapes of tests/test_padding_bits_gpu.py and tests/test_operand_alignment_gpu.py, with the axes on which each needs padding fields
# (snps, indiv): SNP-major rows hold indiv fields, individual-major rows hold snps fields
PADDING_OBJECT_SHAPES = [(67, 261), (270, 526)]            # pitches 17 / 66 bytes; 68 / 132 bytes (multiples of 4: the tiled transpose)
PADDING_XPROD_SHAPES = [(61, 33), (129, 257), (1001, 300)]   # (k fields per row, rows) of the plain crossproduct
PADDING_LD_SHAPES = [(130, 1031), (300, 70)]               # (snps, indiv) of the plain LD entries: SNP-major rows of indiv fields
PADDING_GRM_SHAPES = [(130, 1031), (70, 300)]              # mxa_grm reads individual-major rows of snps fields: 300 SNPs leave no padding field, so the second
                                                           # shape is taken with its axes exchanged
ALIGNMENT_SHAPES = [(272, 528), (270, 526), (67, 261)]     # 4-byte pitches with and without padding fields; ragged pitches


def bits(a):
    """the bit patterns of a float64 / int array (NaNs compare by payload)"""
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])
