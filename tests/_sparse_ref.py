"""sparse_times_plink from its definition, in numpy alone, and the cases both test files use (tests/test_sparse_exact_cpu.py, tests/test_sparse_exact_gpu.py).

The header states the order: for every sparse row j and entry e, acc = 0, then acc = fma(a[t], z[ja[t], e], acc) for t = ia[j] .. ia[j+1] - 1 ascending, with
z in {0, 1, 2}.  a * z is exact in fp64 (|a| <= 2^40 in every case generated here, far from overflow), so the fused multiply-add rounds the same real number
as `acc + a * z` does: chain() below is that loop, vectorised over the entries, and the library is held to it bit for bit.

decode(P, rows, entries)                     packed PLINK rows -> z (rows x entries float64): 00 -> 0, 01 (missing) -> 0, 10 -> 1, 11 -> 2
chain(P, rows, entries, ia, ja, a, ldc)      the documented chain; returns the column-major ldc x entries result as a C-ordered (entries, ldc) array (the
                                             layout of Oracle.sparse_times_plink), zeros in rows nIdx .. ldc - 1.  `mutant` names a planted fault (MUTANTS)
genotypes(rows, entries, seed)               packed rows with about 5 % missing codes, zero padding bits
csr_case(nidx, rows, seed, long_len)         zero-based CSR with every row shape the kernel can meet (see there)
"""
import functools

import numpy as np

MUTANTS = ("reversed", "sorted", "dup_once", "missing_one", "drop_odd_byte", "e_base_ignored")
ORDER_MUTANTS = ("reversed", "sorted")
SLAB = 512                         # columns of the smallest slab of a host C, and the entries of one workgroup


def decode(P, rows, entries, missing=0.0):
    P = np.ascontiguousarray(P, dtype=np.uint8)
    assert P.shape == (rows, (entries + 3) // 4), (P.shape, rows, entries)
    c = np.stack([(P >> (2 * q)) & 3 for q in range(4)], axis=-1).reshape(rows, -1)[:, :entries]
    return np.choose(c, [0.0, missing, 1.0, 2.0])


def pack(codes):
    """codes (rows x entries, values 0 .. 3) -> rows x ceil(entries / 4) bytes, low bits first, zero padding bits"""
    rows, entries = codes.shape
    c = np.zeros((rows, (entries + 3) // 4 * 4), np.uint8)
    c[:, :entries] = codes
    c = c.reshape(rows, -1, 4)
    return np.ascontiguousarray(c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6))


def genotypes(rows, entries, seed, missing=0.05):
    """packed rows: codes 00 / 10 / 11 with probabilities 0.30 / 0.35 / 0.30 and 01 (missing) with 0.05.  The last entry of every row is 10 or 11 (by the
    parity of the row), so that the field the partial last byte -- and, at an odd byte count, the one-byte lane -- ends in is never 0 for all rows; with two or
    more entries, entry 0 of row 0 is the missing code."""
    rng = np.random.default_rng([seed, rows, entries])
    codes = rng.choice(np.array([0, 1, 2, 3], np.uint8), size=(rows, entries), p=[0.35 - missing, missing, 0.35, 0.30])
    codes[:, entries - 1] = 2 + (np.arange(rows) & 1)
    if entries >= 2:
        codes[0, 0] = 1
    return pack(codes)


def chain(P, rows, entries, ia, ja, a, ldc=None, mutant=None):
    assert mutant is None or mutant in MUTANTS, mutant
    ia, ja, a = np.asarray(ia), np.asarray(ja), np.asarray(a, dtype=np.float64)
    nidx = len(ia) - 1
    ldc = nidx if ldc is None else ldc
    assert ldc >= nidx
    Z = decode(P, rows, entries, missing=1.0 if mutant == "missing_one" else 0.0)
    nbytes = (entries + 3) // 4
    if mutant == "drop_odd_byte" and nbytes % 2:        # the lane whose second byte does not exist reads nothing
        Z[:, 4 * (nbytes - 1):] = 0.0
    if mutant == "e_base_ignored":                      # every slab behind the first reads the first slab's bytes
        Z = Z[:, np.arange(entries) % SLAB]
    C = np.zeros((entries, ldc))
    with np.errstate(invalid="ignore", over="ignore"):  # inf * 0 and inf - inf are NaN, as in the kernel
        for j in np.flatnonzero(np.diff(ia)):
            ts = np.arange(ia[j], ia[j + 1])
            if mutant == "reversed":
                ts = ts[::-1]
            elif mutant == "sorted":
                ts = ts[np.argsort(ja[ts], kind="stable")]
            elif mutant == "dup_once":
                ts = ts[np.sort(np.unique(ja[ts], return_index=True)[1])]
            acc = np.zeros(entries)
            for t in ts:
                acc = acc + a[t] * Z[ja[t]]
            C[:, j] = acc
    return C


def values(rng, k):
    """N(0, 1) * 2^k, k uniform in [-20, 20]: the terms of a row span 12 decimal orders, so the order of the additions shows in the bits"""
    return rng.standard_normal(k) * np.exp2(rng.integers(-20, 21, size=k).astype(np.float64))


ROW_KINDS = ("mixed", "empty", "one", "long", "copy", "dup", "ends", "descending")


def csr_case(nidx, rows, seed, long_len=0, kinds=None):
    """zero-based CSR (ia, ja, a) of nidx sparse rows over `rows` packed rows.  Sparse row j has the kind ROW_KINDS[j % 8] (or kinds[j % len(kinds)]):
      mixed       4 .. 16 entries, columns drawn with replacement in random order (unsorted; duplicates happen)
      empty       no entry
      one         one entry
      long        56 .. 64 entries, drawn with replacement
      dup         4 .. 10 distinct columns (as far as there are) in random order, the first two stored again at the end
      ends        4 .. 8 entries that refer to packed rows 0 and rows - 1 only, alternating
      copy        the columns of the nearest earlier non-empty row in reverse order, with new values (duplicates across rows)
      descending  4 .. 16 distinct columns (as far as there are) in descending order
    long_len > 0: row nidx // 2 is replaced by one of long_len entries drawn with replacement.
    About a fifth of the packed rows (never 0 or rows - 1) is referred to by nobody.  Values: values()."""
    rng = np.random.default_rng([seed, nidx, rows])
    inner = np.arange(1, max(rows - 1, 1))
    unused = rng.choice(inner, size=len(inner) // 5, replace=False) if rows >= 7 else np.zeros(0, np.int64)
    allowed = np.setdiff1d(np.arange(rows), unused)
    kinds = kinds or ROW_KINDS
    ia, cols = [0], []
    for j in range(nidx):
        kind = kinds[j % len(kinds)]
        if long_len and j == nidx // 2:
            c = rng.choice(allowed, size=long_len)
        elif kind == "mixed":
            c = rng.choice(allowed, size=int(rng.integers(4, 17)))
        elif kind == "empty":
            c = np.zeros(0, np.int64)
        elif kind == "one":
            c = rng.choice(allowed, size=1)
        elif kind == "long":
            c = rng.choice(allowed, size=int(rng.integers(56, 65)))
        elif kind == "dup":
            c = rng.permutation(allowed)[:int(rng.integers(4, 11))]
            c = np.concatenate([c, c[:2]])
        elif kind == "ends":
            c = np.where(np.arange(int(rng.integers(4, 9))) % 2 == 0, 0, rows - 1)
        elif kind == "copy":
            prev = [p for p in cols if len(p)]
            c = prev[-1][::-1] if prev else rng.choice(allowed, size=3)
        elif kind == "descending":
            c = np.sort(rng.permutation(allowed)[:int(rng.integers(4, 17))])[::-1]
        else:
            raise ValueError(kind)
        cols.append(np.asarray(c, np.int64))
        ia.append(ia[-1] + len(c))
    ja = np.concatenate(cols).astype(np.int32) if ia[-1] else np.zeros(0, np.int32)
    return np.array(ia, np.int32), ja, values(rng, len(ja))


def same_bits(got, want):
    """NaNs in the same places, every other element bit for bit (as _assoc_ref.same_bits)"""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------- the cases of the GPU file
ENTRIES = (1, 3, 4, 5, 7, 8, 9, 511, 512, 513, 1023, 1029)      # partial last bytes; 1 .. 3 bytes; the 512-entry workgroup edge; 129 bytes: the one-byte lane
NIDX = (1, 15, 16, 17, 33)                                      # the 16-row workgroup edge
ROWS = (1, 37, 300)
SLAB_CASE = (1029, 17, 37)                                      # three slabs of 512, 512 and 5 columns


class Case:
    """inputs and the chain's result, read-only"""

    def __init__(self, P, rows, entries, ia, ja, a):
        self.P, self.rows, self.entries, self.ia, self.ja, self.a = P, rows, entries, ia, ja, a
        self.nidx = len(ia) - 1
        for x in (P, ia, ja, a):
            x.setflags(write=False)

    @functools.lru_cache(maxsize=None)
    def want(self, ldc=None, mutant=None):
        C = chain(self.P, self.rows, self.entries, self.ia, self.ja, self.a, ldc=ldc, mutant=mutant)
        C.setflags(write=False)
        return C


@functools.lru_cache(maxsize=None)
def tile_case(entries, nidx, rows):
    """one case of the ENTRIES x NIDX x ROWS grid; nidx = 17 carries a row of 1000 + entries % 7 stored entries"""
    ia, ja, a = csr_case(nidx, rows, seed=101, long_len=1000 + entries % 7 if nidx == 17 else 0)
    return Case(genotypes(rows, entries, seed=7), rows, entries, ia, ja, a)


@functools.lru_cache(maxsize=None)
def nonfinite_case(entries=513, nidx=17, rows=37):
    """the tile case with +inf stored in row 0 and NaN in row 4 (both rows have other entries): inf * 0 = NaN where z is 0, inf elsewhere unless a later term
    makes it NaN"""
    c = tile_case(entries, nidx, rows)
    a = c.a.copy()
    assert c.ia[1] - c.ia[0] >= 2 and c.ia[5] - c.ia[4] >= 2
    a[c.ia[0] + 1] = np.inf
    a[c.ia[4]] = np.nan
    return Case(c.P.copy(), rows, entries, c.ia.copy(), c.ja.copy(), a)


@functools.lru_cache(maxsize=None)
def shape_case(name, entries=513, rows=37):
    """the CSR shapes of their own: all rows empty; one row of 1200 entries (33 packed rows to draw from: duplicates throughout); rows that refer to packed
    row 0 only, to rows - 1 only"""
    rng = np.random.default_rng([5, entries, rows])
    if name == "all_empty":
        ia, ja = np.zeros(18, np.int32), np.zeros(0, np.int32)
    elif name == "single_long":
        ia, ja = np.array([0, 1200], np.int32), rng.integers(0, rows, size=1200).astype(np.int32)
    elif name == "first_only":
        ia, ja = np.arange(0, 18 * 3, 3, dtype=np.int32), np.zeros(17 * 3, np.int32)
    elif name == "last_only":
        ia, ja = np.arange(0, 18 * 3, 3, dtype=np.int32), np.full(17 * 3, rows - 1, np.int32)
    else:
        raise ValueError(name)
    return Case(genotypes(rows, entries, seed=9), rows, entries, ia, ja, values(rng, len(ja)))


SHAPES = ("all_empty", "single_long", "first_only", "last_only")

BIG_BLOCKS = 65535                                              # row blocks of 16 sparse rows in one launch


@functools.lru_cache(maxsize=None)
def big_case():
    """16 * 65535 + 17 sparse rows over 5 entries, nearly all empty: non-empty rows on both sides of the first launch's last row block and at the very end"""
    nidx, rows, entries = 16 * BIG_BLOCKS + 17, 37, 5
    rng = np.random.default_rng(77)
    full = (16 * BIG_BLOCKS - 1, 16 * BIG_BLOCKS, 16 * BIG_BLOCKS + 1, nidx - 1)
    counts = np.zeros(nidx, np.int64)
    counts[list(full)] = (9, 7, 12, 5)
    ia = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    ja = rng.integers(0, rows, size=int(ia[-1])).astype(np.int32)
    return Case(genotypes(rows, entries, seed=11), rows, entries, ia, ja, values(rng, len(ja)))
