"""Shared test helpers: synthetic PLINK data, the oracle (ctypes), the reference driver (build container only).

Everything under oracle/ is TEST INFRASTRUCTURE: loaded here, by __graft_entry__.smoke() and by bench.py's
cpu_baseline leg only.
"""
import ctypes
import os
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
ORACLE_SO = os.environ.get("ORACLE_SO", os.path.join(ORACLE_DIR, "liboracle.so"))   # ORACLE_SO: the sanitizer build (tools/run_sanitizers.sh)
REF_SO = os.path.join(ORACLE_DIR, "_ref", "libmiraculix_ref.so")
REF_DRIVER = os.path.join(ORACLE_DIR, "_ref", "ref_driver")

c_u8p = ctypes.POINTER(ctypes.c_uint8)
c_f64p = ctypes.POINTER(ctypes.c_double)
c_i32p = ctypes.POINTER(ctypes.c_int32)


def synth_genotypes(snps, indiv, seed=42, missing_frac=0.0):
    """Synthetic genotypes per SURVEY.md 8(d): p_s ~ U(0.1,0.6), g ~ Binomial(2,p_s); returns Z (indiv x snps, int8)
    and a missing mask (or None)."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.6, size=snps)
    Z = rng.binomial(2, p[None, :], size=(indiv, snps)).astype(np.int8)
    miss = None
    if missing_frac > 0:
        miss = rng.random((indiv, snps)) < missing_frac
    return Z, miss


def pack_plink(Z, miss=None):
    """Z (rows x cols int, values 0/1/2) -> PLINK 2-bit rows: 0->00, 1->10, 2->11, missing->01; 4 per byte, low bits first,
    rows padded with zero bits (read_plink.jl:152, SURVEY.md terminology)."""
    rows, cols = Z.shape
    code = np.where(Z == 0, 0, Z + 1).astype(np.uint8)
    if miss is not None:
        code = np.where(miss, 1, code).astype(np.uint8)
    pad = (-cols) % 4
    if pad:
        code = np.concatenate([code, np.zeros((rows, pad), np.uint8)], axis=1)
    c4 = code.reshape(rows, -1, 4)
    return (c4[:, :, 0] | (c4[:, :, 1] << 2) | (c4[:, :, 2] << 4) | (c4[:, :, 3] << 6)).astype(np.uint8)


def make_problem(snps, indiv, n, seed=42, missing_frac=0.0, ldb_pad=0):
    """Returns dict with plink (snps x ceil(indiv/4)), plink_t (indiv x ceil(snps/4)), f, Z (with missing as 0)."""
    Z, miss = synth_genotypes(snps, indiv, seed, missing_frac)
    plink = pack_plink(Z.T.copy(), None if miss is None else miss.T.copy())
    plink_t = pack_plink(Z, miss)
    Zeff = Z.copy()
    if miss is not None:
        Zeff[miss] = 0
    f = Zeff.astype(np.float64).mean(axis=0) / 2.0
    return dict(snps=snps, indiv=indiv, plink=np.ascontiguousarray(plink), plink_t=np.ascontiguousarray(plink_t), f=f, Z=Zeff)


def make_B(k, n, seed=43, ldb=None):
    rng = np.random.default_rng(seed)
    ldb = ldb or k
    B = np.zeros((n, ldb))  # row j = column j of the column-major matrix
    B[:, :k] = rng.standard_normal((n, k))
    if ldb > k:
        B[:, k:] = 1e300  # poison the ld padding: must never be read as data
    return B


def elementwise_bound(o, trans, prob, B, centered, factor=4.0):
    """The hard element-wise error bound of SURVEY.md 8(d) for an fp64 chain of length K: factor * K * 2^-53 * sum_k |z_ik| |b_kj|, per output (n x m, like
    Oracle.dgemm_dense).  Centred: the product computes sum z b and the rank-1 term 2 sum f b separately, so the magnitudes add: 'N' + 2 sum_k f_k |b_kj| (per
    column), 'T' + 2 f_s sum_i |b_ij|.  The norm-wise tolerance (1e-11 of the largest entry) leaves output rows far below max|C| unprotected; this one does not."""
    snps, indiv = prob["snps"], prob["indiv"]
    k, m = (indiv, snps) if trans else (snps, indiv)
    Ba = np.ascontiguousarray(np.abs(B))
    mag = o.dgemm_dense(trans, prob, Ba, 0)[:, :m]                                   # sum |z| |b|  (z >= 0)
    if centered:
        f = np.asarray(prob["f"], dtype=np.float64)
        if trans:
            mag = mag + 2.0 * Ba[:, :k].sum(axis=1)[:, None] * f[None, :m]
        else:
            mag = mag + 2.0 * (Ba[:, :k] * f[None, :k]).sum(axis=1)[:, None]
    return factor * k * 2.0 ** -53 * mag


class Oracle:
    def __init__(self):
        if not os.path.exists(ORACLE_SO):
            subprocess.check_call(["make", "-C", ORACLE_DIR, "liboracle.so"])
        L = ctypes.CDLL(ORACLE_SO)
        self.L = L
        L.oracle_dgemm_dense.argtypes = [ctypes.c_int, c_u8p, ctypes.c_long, ctypes.c_long, c_f64p, ctypes.c_int, ctypes.c_long, c_f64p, ctypes.c_long, c_f64p, ctypes.c_long]
        L.oracle_dgemm_gpuorder.argtypes = [ctypes.c_int, c_u8p, c_u8p, ctypes.c_long, ctypes.c_long, c_f64p, ctypes.c_int, ctypes.c_long, c_f64p, ctypes.c_long, c_f64p, ctypes.c_long]
        L.oracle5_create.restype = ctypes.c_void_p
        L.oracle5_create.argtypes = [c_u8p, ctypes.c_long, ctypes.c_long, c_f64p, ctypes.c_int]
        L.oracle5_dgemm.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_long, c_f64p, ctypes.c_long, c_f64p, ctypes.c_long]
        L.oracle5_free.argtypes = [ctypes.c_void_p]
        L.oracle_crossprod_i32.argtypes = [c_u8p, ctypes.c_long, ctypes.c_long, ctypes.c_int, c_i32p]
        L.oracle_crossprod_f64.argtypes = [c_u8p, ctypes.c_long, ctypes.c_long, ctypes.c_int, c_f64p]
        L.oracle_transpose_2bit.argtypes = [c_u8p, ctypes.c_long, ctypes.c_long, c_u8p]
        L.oracle_allele_freq.argtypes = [c_u8p, ctypes.c_long, ctypes.c_long, c_f64p]
        L.oracle_num_threads.restype = ctypes.c_int
        L.oracle_sparse_times_plink.argtypes = [c_u8p, ctypes.c_long, ctypes.c_long, ctypes.c_int, c_i32p, c_i32p, c_f64p, c_f64p, ctypes.c_long]

    @staticmethod
    def _u8(a):
        return a.ctypes.data_as(c_u8p)

    @staticmethod
    def _f64(a):
        return a.ctypes.data_as(c_f64p)

    def dgemm_dense(self, trans, prob, B, centered, ldc=None):
        snps, indiv = prob["snps"], prob["indiv"]
        n, ldb = B.shape
        m = snps if trans else indiv
        ldc = ldc or m
        C = np.full((n, ldc), -777.0)
        self.L.oracle_dgemm_dense(int(trans), self._u8(prob["plink"]), snps, indiv, self._f64(prob["f"]), int(centered), n, self._f64(B), ldb, self._f64(C), ldc)
        return C

    def dgemm_gpuorder(self, trans, prob, B, centered, ldc=None):
        snps, indiv = prob["snps"], prob["indiv"]
        n, ldb = B.shape
        m = snps if trans else indiv
        ldc = ldc or m
        C = np.full((n, ldc), -777.0)
        self.L.oracle_dgemm_gpuorder(int(trans), self._u8(prob["plink"]), self._u8(prob["plink_t"]), snps, indiv, self._f64(prob["f"]), int(centered), n, self._f64(B), ldb, self._f64(C), ldc)
        return C

    def five_create(self, prob, cores=0):
        cores = cores or self.L.oracle_num_threads()
        return self.L.oracle5_create(self._u8(prob["plink"]), prob["snps"], prob["indiv"], self._f64(prob["f"]), cores)

    def five_dgemm(self, h, trans, prob, B, centered, ldc=None):
        n, ldb = B.shape
        m = prob["snps"] if trans else prob["indiv"]
        ldc = ldc or m
        C = np.full((n, ldc), -777.0)
        self.L.oracle5_dgemm(h, int(trans), int(centered), n, self._f64(B), ldb, self._f64(C), ldc)
        return C

    def five_free(self, h):
        self.L.oracle5_free(h)

    def crossprod_i32(self, X, k, is_plink):
        rows = X.shape[0]
        out = np.zeros((rows, rows), np.int32)
        self.L.oracle_crossprod_i32(self._u8(X), k, rows, int(is_plink), out.ctypes.data_as(c_i32p))
        return out

    def transpose_2bit(self, X, rows, cols):
        out = np.zeros((cols, (rows + 3) // 4), np.uint8)
        self.L.oracle_transpose_2bit(self._u8(X), rows, cols, self._u8(out))
        return out

    def sparse_times_plink(self, P, rows, entries, ia, ja, a, ldc=None):
        """P: rows x ceil(entries/4) PLINK bytes; (ia, ja, a): zero-based CSR with len(ia)-1 sparse rows.  Returns the column-major
        C as numpy (entries, ldc)."""
        nidx = len(ia) - 1
        ldc = ldc or nidx
        C = np.full((entries, ldc), -777.0)
        ia = np.ascontiguousarray(ia, np.int32); ja = np.ascontiguousarray(ja, np.int32); a = np.ascontiguousarray(a, np.float64)
        self.L.oracle_sparse_times_plink(self._u8(P), rows, entries, nidx, ia.ctypes.data_as(c_i32p), ja.ctypes.data_as(c_i32p), self._f64(a), self._f64(C), ldc)
        return C

    def allele_freq(self, plink, snps, indiv):
        f = np.zeros(snps)
        self.L.oracle_allele_freq(self._u8(plink), snps, indiv, self._f64(f))
        return f


def random_csr(nidx, ncols, max_nnz, seed, empty_rows=True):
    """Zero-based CSR (ia, ja, a) with 0..max_nnz sorted distinct columns per row and N(0,1) values."""
    rng = np.random.default_rng(seed)
    ia, ja, a = [0], [], []
    for j in range(nidx):
        k = int(rng.integers(0 if empty_rows else 1, min(max_nnz, ncols) + 1))
        cols = np.sort(rng.choice(ncols, size=k, replace=False))
        ja += cols.tolist()
        a += rng.standard_normal(k).tolist()
        ia.append(len(ja))
    return np.array(ia, np.int32), np.array(ja, np.int32), np.array(a, np.float64)


def have_reference():
    return os.path.exists(REF_SO) and os.path.exists(REF_DRIVER)


def run_reference(prob, trans, B, centered, ldc=None, variant=256, cores=8, reps=1):
    """Run the reference's own CPU 5codes library (oracle/_ref, build container or wherever it was built)."""
    snps, indiv = prob["snps"], prob["indiv"]
    n, ldb = B.shape
    m = snps if trans else indiv
    ldc = ldc or m
    with tempfile.TemporaryDirectory() as td:
        fin, fout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(fin, "wb") as fh:
            fh.write(struct.pack("9i", snps, indiv, n, ldb, ldc, int(trans), int(not centered), variant, cores))
            fh.write(prob["plink"].tobytes())
            fh.write(prob["f"].astype(np.float64).tobytes())
            fh.write(np.ascontiguousarray(B).tobytes())
        env = dict(os.environ, OMP_NUM_THREADS=str(cores))
        subprocess.run([REF_DRIVER, REF_SO, fin, fout, str(reps)], check=True, env=env, stdout=subprocess.DEVNULL, timeout=600)
        raw = np.fromfile(fout, dtype=np.float64)
    C = raw[: n * ldc].reshape(n, ldc)
    return C, float(raw[n * ldc])


# ====================================================================================================== sampled-rows checker of the tests
# A checker of its own for the full-size fp64 tests, independent of bench.py's check_sample (which the bench legs use): the sampled packed rows are
# unpacked here with numpy, the reference is summed here in long double, and the "got" values are read from C by one gather of (row, column) pairs.
SAMPLE_RTOL = 1e-11   # stated fp64 tolerance of the dgemm path: max|C - C_ref| <= 1e-11 max|C_ref|


def unpack_2bit(P, k, is_plink=True):
    """packed rows (rows x ceil(k/4) uint8, 4 fields per byte, low bits first) -> rows x k int8.  PLINK codes decode as the dgemm path reads them:
    00 -> 0, 01 (missing) -> 0, 10 -> 1, 11 -> 2; raw fields are the values."""
    P = np.ascontiguousarray(P, dtype=np.uint8)
    V = np.stack([(P >> (2 * q)) & 3 for q in range(4)], axis=-1).reshape(P.shape[0], -1)[:, :k]
    if is_plink:
        V = np.where(V >= 2, V - 1, 0)
    return V.astype(np.int8)


def _to_numpy(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def take_sample(torch, S, nsample, seed):
    """nsample individuals (rows of the individual-major S["plink_t"]) and nsample SNPs (rows of the SNP-major S["plink"]) chosen by a generator
    seeded with `seed`, their packed rows copied to the host.  S: dict(snps, indiv, plink, plink_t, f) with device tensors."""
    snps, indiv = S["snps"], S["indiv"]
    rng = np.random.default_rng(seed)
    ii = np.sort(rng.choice(indiv, min(nsample, indiv), replace=False))
    ss = np.sort(rng.choice(snps, min(nsample, snps), replace=False))
    rows_t = S["plink_t"].index_select(0, torch.as_tensor(ii, device=S["plink_t"].device))
    rows_s = S["plink"].index_select(0, torch.as_tensor(ss, device=S["plink"].device))
    return dict(snps=snps, indiv=indiv, f=_to_numpy(S["f"]), ii=ii, ss=ss, rows_t=_to_numpy(rows_t), rows_s=_to_numpy(rows_s))


def check_sampled_rows(sample, trans, B, C, cols, centered, row_offset=0, rtol=SAMPLE_RTOL):
    """Sampled rows of C = op(Z - 2 f 1^T) B ('N': C indiv x n, rows = individuals sample["ii"] from sample["rows_t"]; 'T': C snps x n, rows = SNPs
    sample["ss"] from sample["rows_s"]), columns `cols`, against a long-double sum over the numpy-unpacked packed rows.  C (numpy or torch, any strides)
    may be the row block of the result that starts at row `row_offset`.  Returns dict(err = max|got - ref| / max|ref|, bound_ratio = max over the sampled
    elements of |got - ref| / elementwise_bound (4 K 2^-53 times the magnitude of the sum), ok = err <= rtol and bound_ratio <= 1).  The long-double
    reference is within K 2^-64 of that magnitude: 1/8192 of the bound."""
    snps, indiv = sample["snps"], sample["indiv"]
    f = _to_numpy(sample["f"]).astype(np.float64)
    cols = np.asarray(cols, dtype=np.int64)
    Bs = _to_numpy(B[:, [int(c) for c in cols]] if hasattr(B, "detach") else np.asarray(B)[:, cols]).astype(np.float64)    # k x len(cols)
    if not trans:
        rows, k = np.asarray(sample["ii"]), snps
        Z = unpack_2bit(sample["rows_t"], snps)                                       # nsample x snps
        shift = np.broadcast_to(2.0 * f.astype(np.longdouble)[None, :], Z.shape)      # z_is - 2 f_s
    else:
        rows, k = np.asarray(sample["ss"]), indiv
        Z = unpack_2bit(sample["rows_s"], indiv)                                      # nsample x indiv
        shift = np.broadcast_to(2.0 * f[rows].astype(np.longdouble)[:, None], Z.shape)   # z_si - 2 f_s
    assert Bs.shape[0] == k, (Bs.shape, k)
    Bl = Bs.astype(np.longdouble)
    ref = np.empty((len(rows), len(cols)), dtype=np.float64)
    for q in range(len(rows)):
        zc = Z[q].astype(np.longdouble) - (shift[q] if centered else 0.0)
        ref[q] = (zc @ Bl).astype(np.float64)
    r = rows - row_offset
    if hasattr(C, "detach"):
        import torch
        got = C[torch.as_tensor(r, device=C.device)[:, None], torch.as_tensor(cols, device=C.device)[None, :]].cpu().numpy()
    else:
        got = np.asarray(C)[r[:, None], cols[None, :]]
    diff = np.abs(got - ref)
    err = float(diff.max() / np.abs(ref).max()) if np.abs(ref).max() > 0 else float(diff.max())
    # the hard element-wise bound on the sub-problem of the sampled rows (SNP-major packing of the unpacked values)
    if not trans:
        prob = dict(snps=snps, indiv=len(rows), plink=pack_plink(np.ascontiguousarray(Z.T)), f=f)
    else:
        prob = dict(snps=len(rows), indiv=indiv, plink=pack_plink(Z), f=np.ascontiguousarray(f[rows]))
    bound = elementwise_bound(Oracle(), trans, prob, np.ascontiguousarray(Bs.T), centered).T        # nsample x len(cols)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, diff / bound, np.where(diff == 0, 0.0, np.inf))
    ratio = float(ratio.max())
    ok = bool(np.all(np.isfinite(got)) and err <= rtol and ratio <= 1.0)
    return dict(err=err, bound_ratio=ratio, ok=ok)


def second_opinion_on_check_sample(monkeypatch, bench):
    """Wrap bench.check_sample (through monkeypatch) so that every (B, C) a bench leg checks also goes through check_sampled_rows, on the same sample
    and the same columns; returns the list the verdicts are appended to.  The leg's own result is returned unchanged."""
    verdicts = []
    orig = bench.check_sample

    def both(torch, sample, trans, Bdev, Cdev, cols, centered, row_offset=0, want_bound=False):
        out = orig(torch, sample, trans, Bdev, Cdev, cols, centered, row_offset=row_offset, want_bound=want_bound)
        v = check_sampled_rows(sample, trans, Bdev, Cdev, cols, centered, row_offset=row_offset)
        verdicts.append(dict(v, trans=int(trans), rows=len(sample["ss"] if trans else sample["ii"]), cols=list(cols)))
        return out

    monkeypatch.setattr(bench, "check_sample", both)
    return verdicts
