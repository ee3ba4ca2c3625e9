/* miraculix_amd.h -- C ABI of the MI355X-native compressed-genotype GEMM engine.
 *
 * Part 1 is the drop-in boundary: exactly the unmangled C symbols the reference's language bindings
 * bind (dlopen + ccall in src/bindings/Julia/{dgemm_compressed,crossproduct}.jl, bind(C) in src/bindings/Fortran/mod5codesapi.f90).
 * Each declaration cites the reference interface it replaces (paths relative to the reference repo).
 * Part 2 are additive entry points (prefix mxa_) for device-resident operands, SNP-sharded multi-GPU
 * use, on-device .bed staging helpers and measurement; the reference has no counterpart for them.
 *
 * All matrices are column-major fp64.  Plain pointers and sizes only.
 *
 * ALIGNMENT.  Every pointer argument is valid at the natural alignment of its element type -- 1 byte for packed genotypes and keep[], 4 for int, 8 for double
 * and long -- in host or in device memory, and no result depends on it: base + 3 of a memory-mapped .bed, a slice of a device tensor, a column of a bigger
 * buffer and a Fortran array section give bit for bit what a fresh allocation gives.  Nothing in front of or behind an output is written.
 *
 * PADDING BITS.  A packed row of k 2-bit fields takes ceil(k / 4) bytes; when k is no multiple of 4 the last byte has fields at and beyond k.  A well-formed
 * .bed has 00 there; a buffer that is reused or sliced may not.  What they mean, by entry group (each group's comment repeats its rule):
 *   ignored    -- plink2compressed, mxa_plink2compressed_shard / _begin / _rows / _end, mxa_bed2compressed(_range) and everything computed from their objects
 *                 (dgemm_compressed, mxa_dgemm_compressed_device / _multi, mxa_gram_matvec(_device), get_compressed_freq); dgemm_plink; sparse_times_plink;
 *                 mxa_transpose_2bit (its output has 00 in its own padding); mxa_allele_freq; mxa_grm, mxa_ld and every mxa_ld_* entry, plain and _pairwise.
 *                 These entries know how many genotypes a row holds; the result is bit for bit that of the same call on 00 padding.
 *   as stored  -- snp_multiply_gpu and mxa_snp_multiply_panel, as in the reference: whole bytes are multiplied, so the padding fields enter the sums with
 *                 the values they hold (under is_plink_format a padding 01 turns its byte into four 3s).  Clear them before the call.
 */
#ifndef MIRACULIX_AMD_H
#define MIRACULIX_AMD_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the entry points declared in this header are exported (no C++ symbol of the
 * implementation reaches the namespace of the Julia / R / Fortran process that loads it). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ------------------------------------------------------------------ Part 1: reference ABI */

/* replaces src/miraculix/5codesAPI.c:43-70 (prototype src/miraculix/5codes.h:137-153; doc
 * docs/genotype_matrix_multiplication.md:5-17; Fortran binding src/bindings/Fortran/mod5codesapi.f90:22-40).
 * Process-global options.  This engine is GPU-only: use_gpu == 0 prints a message, sets mxa_last_error() (code 14) and
 * makes every later plink2compressed leave its handle NULL until setOptions_compressed is called again with use_gpu != 0 --
 * the host process (a Julia / R session) is not terminated and no CPU engine is substituted.  The combinations the
 * reference rejects for its GPU path (5codesChar.cc:192-193: use_miraculix_freq != 0, ignore_missings == 0,
 * do_normalize != 0) are fatal (stderr + exit) exactly as there.  cores, floatLoop, meanSubstract, variant have no GPU meaning and are
 * accepted and ignored (src/miraculix/GPUapi.h:38). */
void setOptions_compressed(int use_gpu, int cores, int floatLoop, int meanSubstract, int ignore_missings,
                           int do_not_center, int do_normalize, int use_miraculix_freq, int variant,
                           int print_details);

/* replaces src/miraculix/5codesAPI.c:80-96 -> plink2gpu (src/cuda/dgemm_compressed_cuda.cu:43-170).
 * plink: SNP-major bed payload without the 3 header bytes, snps rows of ceil(indiv/4) bytes;
 * plink_transposed: indiv rows of ceil(snps/4) bytes; f: snps allele frequencies (required when centring);
 * max_n: largest n later passed to dgemm_compressed (buffers grow if exceeded).  The data is copied: the caller
 * may free its buffers afterwards.  Either matrix pointer may also be a device pointer.
 * plink_transposed may be NULL or the same pointer as plink -- the call shape of the reference's CPU path, which never reads it
 * (5codesChar.cc:368-393; utils/benchmark/benchmark.f90:185 passes the same pointer twice): then only the SNP-major matrix is uploaded
 * and the individual-major copy is produced on the device (2-bit transpose of the raw PLINK codes), bit-identical to the object built
 * from two pointers.  On failure *compressed is left NULL and a message is printed (reference: print + handle unset).
 * Padding bits: IGNORED in both matrices (fields at and beyond indiv of a SNP-major row, at and beyond snps of an individual-major row), for every call
 * shape and for the other staging entries (mxa_plink2compressed_shard, _begin / _rows / _end, mxa_bed2compressed(_range)); so are they by every product of the
 * object and by get_compressed_freq.
 * A host matrix is uploaded in row chunks through a bounce buffer of 256 MB, or of MXA_STAGE_CHUNK_ROWS rows (a test knob, read per call; so do
 * mxa_plink2compressed_shard, mxa_plink2compressed_rows and dgemm_plink): results are bit-identical for every chunk size. */
void plink2compressed(char *plink, char *plink_transposed, int snps, int indiv, double *f, int max_n,
                      void **compressed);

/* replaces src/miraculix/5codesAPI.c:98-110 -> dgemm_compressed_gpu (src/cuda/dgemm_compressed_cuda.cu:218-489).
 * trans[0] in {N,n}: C(indiv x n) = (Z - 2*1*f^T) * B(snps x n); {T,t,Y,y}: C(snps x n) = (Z - 2*1*f^T)^T * B(indiv x n);
 * anything else: exit(99) (5codesAPI.c:73-77).  Centring is governed by do_not_center.  Ldb/Ldc are honoured
 * (the reference GPU path ignores them, its CPU path honours them and zero-fills the padding rows of C;
 * so does this).  B and C may each be host or device pointers.  Synchronous. */
void dgemm_compressed(char *trans, void *compressed, int n, double *B, int Ldb, double *C, int Ldc);

/* replaces src/miraculix/5codesAPI.c:159-161 -> freegpu (src/cuda/dgemm_compressed_cuda.cu:176-213).
 * Releases all device memory and sets *compressed = NULL (the reference leaves the caller's pointer dangling). */
void free_compressed(void **compressed);

/* replaces src/miraculix/5codesAPI.c:37-39.  Returns the allele frequencies stored with the object. */
void get_compressed_freq(void *compressed, double *f);

/* replaces src/miraculix/5codesAPI.c:135-157 -> sparseTGenoPlinkApi (5codesChar.cc:472-491) -> sparseTGenoPlink
 * (plinkUint.cc:352-470); Fortran binding src/bindings/Fortran/mod5codesapi.f90:84-100, caller
 * tests/sparse_plink/test_sparse_plink.f90:99.  Sparse (CSR) times packed genotypes, uncentred, missing -> 0.  Behaviour as
 * observed from the reference's library (golden fixtures in tests/golden/sparse_golden.npz): the sparse COLUMN index selects a row
 * of the packed matrix and the result runs over the 2-bit entries of that row --
 *   transcompressed in {N,n}: C (nIdx x indiv, ld Ldc) = S (nIdx x snps)  * Z^T, packed matrix = plink;
 *   transcompressed in {T,t,Y,y}: C (nIdx x snps, ld Ldc) = S (nIdx x indiv) * Z, packed matrix = plink_transposed.
 * rowIdxB (nIdx + 1 entries) / colIdxB / B are ZERO-based CSR; C is zero-filled over Ldc x columns, also when nIdx == 0 (as the
 * reference, which clears C before it looks at nIdx).  The columns of a sparse row need not be sorted or distinct: a column stored
 * twice is added twice.  nIdx is bounded by int alone.  transsparse must be N (the reference aborts otherwise; so does this).  Only
 * the packed matrix that is used needs to be non-NULL.  Each of the packed matrix, rowIdxB, colIdxB, B and C may be a host or a
 * device pointer, independently.  Padding bits of the packed rows: IGNORED.
 * Summation order: CSR order, one fused multiply-add per stored entry --
 *     acc = 0;  for t = rowIdxB[j] .. rowIdxB[j+1]-1 ascending:  acc = fma(B[t], z(colIdxB[t], e), acc);  C[j + e*Ldc] = acc
 * with z in {0, 1, 2} (00 -> 0, 01 = missing -> 0, 10 -> 1, 11 -> 2).  B[t] * z is exact, so every element is the plain
 * left-to-right fp64 sum of its row's terms: the same bits from run to run, for every pointer kind and for every piece size of the
 * host staging.  A host packed matrix is uploaded as the rows S refers to, through a bounce buffer of 256 MiB or
 * MXA_SPARSE_CHUNK_BYTES bytes (at least one row); a host C leaves through a device buffer of 1 GiB or MXA_SPARSE_SLAB_BYTES
 * bytes, in slabs of a multiple of 512 columns (at least 512).  Both variables are read per call; under PRINT_LEVEL > 0 the call
 * prints how many chunks and slabs it ran in.
 * Errors (message on stderr, C unwritten, mxa_last_error() != 0): a NULL packed matrix, rowIdxB or C, snps or indiv < 1,
 * nIdx < 0, rowIdxB[0] != 0, rowIdxB decreasing, NULL colIdxB or B with stored entries, a column outside [0, rows): 1;
 * Ldc < nIdx: 7. */
void sparse_times_plink(char *transsparse, char *transcompressed, char *plink, char *plink_transposed, int snps, int indiv,
                        int nIdx, int *rowIdxB, int *colIdxB, double *B, double *C, int Ldc);

/* replaces src/miraculix/5codesAPI.c:112-130 (prototype 5codes.h:137-153 region; docs/genotype_matrix_multiplication.md) -> vectorGenoPlinkApi
 * (5codesChar.cc:495-520).  One product straight from the PLINK matrices, no object kept: the DOCUMENTED semantics -- trans in {N,n}: C (indiv x n)
 * = Zc B with B snps x n; {T,t,Y,y}: C (snps x n) = Zc^T B with B indiv x n; f != NULL: centred with the caller's frequencies, f == NULL: uncentred
 * (whatever setOptions_compressed says) -- as the composition plink2compressed + dgemm_compressed + free_compressed of this library.
 * PARITY UNPINNED: in the reference this entry ends in an unconditional BUG abort for every input (f != NULL: 5codesChar.cc:511-513; f == NULL:
 * plink256.cc:332) and nothing binds it, so there is no reference output to compare with; results are checked against the dense oracle.  The reference's
 * "indiv must be a multiple of 32" (5codesChar.cc:510) is not required.  Only the matrix the reference would read needs to be non-NULL ('N':
 * plink_transposed, 'T': plink); when only plink_transposed is given it is transposed on the device first.  Host or device pointers.
 * Padding bits: IGNORED, as by plink2compressed.  Errors: message on stderr, C unwritten, mxa_last_error() != 0. */
void dgemm_plink(char *trans, char *plink, char *plink_transposed, int snps, int indiv, double *f, int n, double *B, int Ldb, double *C, int Ldc);

/* replaces src/cuda/snp_multiply_cuda.cu:375-382 (prototype src/cuda/snp_multiply_cuda.h:113-114; Julia binding
 * src/bindings/Julia/crossproduct.jl:54-58, which passes the bool as Cint).
 * ans(indiv x indiv, column-major doubles, full symmetric) = X * X^T where X has `indiv` rows of ceil(snps/4) bytes
 * of 2-bit values; positional meaning as in the reference: `snps` = packed (inner) dimension, `indiv` = output
 * dimension.  is_plink_format applies the reference's byte table first (00->0, 10->1, 11->2, any byte holding a
 * missing 01 pair -> 0xFF).  Exact int32 accumulation.  snp_matrix and ans may be host or device pointers.
 * Padding bits: AS STORED.  The reference multiplies whole bytes (snp_multiply_cuda.h:121-210), and so does this: when snps is no multiple of 4, the fields
 * at and beyond snps of a row's last byte are multiplied like genotypes (and a 01 among them makes the byte 0xFF under the table).
 * A host snp_matrix is uploaded in row chunks through a bounce buffer of 256 MiB, or of MXA_STAGE_CHUNK_ROWS rows (a test knob, read per call; so do
 * mxa_snp_multiply_panel, mxa_grm, mxa_ld and every windowed-LD entry that takes the packed matrix): results are bit-identical for every chunk size.
 * Returns 0 on success, 1 on failure. */
int snp_multiply_gpu(unsigned char *snp_matrix, int snps, int indiv, double *ans, bool is_plink_format);

/* ---- solver twin (not on the compressed-genotype hot path) behind the reference's solver exports
 * src/cuda/solve_cuda.cu:927-951 (prototypes src/cuda/solve_cuda.h:61-88; Julia binding src/bindings/Julia/solve.jl:45-180;
 * Fortran binding src/bindings/Fortran/modmiraculix_gpu.f90:23-80).  Blocked Cholesky and a synchronisation-free sparse
 * triangular solve written here, Level-3 updates on the fp64 matrix cores included (no vendor library is loaded).  All matrices column-major fp64;
 * pointers may be host or device. */

/* replaces solve_cuda.cu:947-951 -> dense_solve (:70-280): X = A^-1 B by Cholesky (lower triangle of the symmetric positive
 * definite A, input_size x input_size; B, X input_size x rhs_cols) and, if logdet != NULL, *logdet = log det A = sum 2 log L_ii.
 * oversubscribe: 1 = the matrix lives in managed memory (hipMallocManaged), 0 = device memory; anything else is an error.
 * *status = 0 on success, 1 on failure (message on stderr; a matrix that is not positive definite reports the failing minor). */
void potrs_solve_gpu(double *A, unsigned int input_size, double *B, unsigned int rhs_cols, double *X, double *logdet,
                     int oversubscribe, int *status);
/* replaces solve_cuda.cu:927-931: the same, status as the return value */
int potrs_solve(double *A, unsigned int input_size, double *B, unsigned int rhs_cols, double *X, double *logdet,
                int oversubscribe);

/* replaces solve_cuda.cu:933-936 -> sparse_solve_init (:281-578): stage a sparse triangular m x m matrix given as ONE-based COO
 * triplets (V, I, J; 64-bit indices; any order -- they are sorted into CSR here) for solves with exactly `ncol` right-hand
 * sides; is_lower != 0: lower triangular, else upper.  *GPU_obj receives the object (NULL on failure), *status 0 / 1. */
void sparse2gpu(double *V, long *I, long *J, long nnz, long m, long ncol, int is_lower, void **GPU_obj, int *status);
/* replaces solve_cuda.cu:938-941 -> sparse_solve_compute (:709-880): X (m x ncol) = op(A)^-1 B, transA in {N,n}: op(A) = A,
 * {T,t,f}: op(A) = A^T (as the reference); ncol must equal the value given to sparse2gpu. */
void dcsrtrsv_solve_gpu(void *GPU_obj, char transA, double *B, long ncol, double *X, int *status);
/* replaces solve_cuda.cu:943-945 -> sparse_solve_destroy (:580-707): releases the object and sets *GPU_obj = NULL (the Julia
 * test expects a second free to be caught by its NULL check, tests/solve/test.jl:129). */
void free_sparse_gpu(void **GPU_obj, int *status);

/* ------------------------------------------------------------------ Part 2: additive entry points */

/* status of the most recent fallible API call of the process: 0 = it succeeded (every such entry clears the status first);
 * the message is valid until the next call. */
int mxa_last_error(void);
const char *mxa_last_error_string(void);

/* number of visible HIP devices, or -1 if the runtime cannot be initialised */
int mxa_device_count(void);

/* SNP-sharded staging for one-process-per-GPU use: like plink2compressed, but this object holds only SNPs
 * [snp_begin, snp_end) of the full matrix.  plink points at the FULL SNP-major payload (row pitch ceil(indiv/4));
 * plink_transposed at the FULL individual-major payload (row pitch ceil(snps_total/4)); f at the FULL frequency
 * vector.  snp_begin must be a multiple of 4 so that packed bytes split cleanly.
 * For 'N' the caller passes rows [snp_begin, snp_end) of B and sum-reduces C over the shards
 * (the centring term is a partial sum too and rides along); for 'T' C holds rows [snp_begin, snp_end).
 * plink_transposed may be NULL (or == plink): the shard transposes its own SNP block on the device. */
void mxa_plink2compressed_shard(char *plink, char *plink_transposed, int snps_total, int indiv, int snp_begin,
                                int snp_end, double *f, int max_n, void **compressed);

/* dgemm_compressed with 64-bit leading dimensions on an explicit HIP stream (NULL = the object's own stream),
 * device pointers only, asynchronous when sync == 0.  Returns 0 / 1.
 * Asynchronous for EVERY n under the default engine (round 5): the verdict of the exact int8 route of narrow products and peeled columns is formed on
 * the device; nothing is read back.  (The first call of a new shape on an object may grow its workspace, which waits for the stream once; the opt-in
 * engine `i8-exact` reads three integers per call, as documented with it.)
 * ONE CALL IN FLIGHT PER OBJECT: every multiply on an object uses that object's workspace (fragment-ordered B, split-K
 * partials, column sums).  Calls on the same object must therefore be serialised on ONE stream (or the caller must wait
 * for the previous call before issuing the next on another stream); this includes mxa_gram_matvec and dgemm_compressed.
 * Different objects are independent.  Not available on multi-device objects (MIRACULIX_NUM_GPUS > 1). */
int mxa_dgemm_compressed_device(char trans, void *compressed, int n, const double *dB, long ldb, double *dC,
                                long ldc, void *hip_stream, int sync);

/* one step of the GRM-based solvers (reference loop: examples/iterative_solver/grm_solve_cg.jl:74-84, which calls
 * dgemm_compressed 'T' then 'N' and notes the cost of moving the operands each time at dgemm_compressed_cuda.cu:251-252):
 * out (indiv x n, ld ldo) = Zc * (Zc^T * V), V indiv x n (ld ldv); the snps x n intermediate stays in HBM.  Centring as set by
 * setOptions_compressed.  V / out host or device.  On a SNP shard the result is that shard's partial sum.  Returns 0 / 1. */
int mxa_gram_matvec(void *compressed, int n, const double *V, long ldv, double *out, long ldo);
/* the same with device-resident V / out (memory of the object's device) and optional asynchrony: sync == 0 returns when both products are
 * enqueued on the object's stream -- a blocking stream, so work the caller enqueues afterwards on the device's default stream (PyTorch, hipBLAS
 * on stream 0) is ordered behind it and a CG / GBLUP loop on device-resident vectors never waits on the host: the ~40 us between two
 * synchronous calls (return, caller, next launch) disappear from every iteration.  Single-device objects only.  Returns 0 / 1.
 * (No n waits on the host under the default engine: see mxa_dgemm_compressed_device.) */
int mxa_gram_matvec_device(void *compressed, int n, const double *dV, long ldv, double *dOut, long ldo, int sync);

/* on-device .bed staging helpers (reference counterparts live in the bindings:
 * transpose_genotype_matrix src/bindings/Julia/compressed_operations.jl:45-66, popcount frequencies
 * src/bindings/Julia/read_plink.jl:199-203).  Pointers may be host or device.
 * Padding bits: IGNORED by both; the rows mxa_transpose_2bit writes have 00 in their own padding fields, whatever the input's held. */
int mxa_transpose_2bit(const unsigned char *in, long rows, long cols, unsigned char *out);
/* f_s = (sum of the allele counts of SNP s) / (2 indiv) with the decode the multiply uses: 00 -> 0, 10 -> 1, 11 -> 2 and the
 * missing code 01 -> 0, so that f is exactly the column mean / 2 of the matrix dgemm_compressed multiplies with.
 * DEVIATION on data with missing genotypes: the reference binding counts set bits (read_plink.jl:199-203), i.e. a missing
 * 01 adds 1; on missing-free data (the only data the reference's tests and crossproduct accept, read_plink.jl:213) both agree. */
int mxa_allele_freq(const unsigned char *plink, long snps, long indiv, double *f);

/* PLINK .bed staging owned by the library: reads the SNP-major .bed file `bed_path` (3-byte magic 6c 1b 01, then snps rows of
 * ceil(indiv/4) bytes; reference reader: src/bindings/Julia/read_plink.jl:161-222), uploads it in chunks, builds the
 * individual-major copy with the on-device 2-bit transpose and the allele frequencies with the on-device popcount
 * (f_s = allele count / (2 indiv)), and returns the same kind of object as plink2compressed.  snps / indiv <= 0: taken
 * from the line counts of the .bim / .fam files next to the .bed.  f_out (optional, host, snps doubles) receives the
 * frequencies; snps_out / indiv_out (optional) the dimensions.  Returns 0 / 1; *compressed is NULL on failure.
 * The file is read in chunks of 64 MiB, or of MXA_STAGE_CHUNK_ROWS rows (a test knob, read per call, also by mxa_bed2compressed_range and the in-process
 * sharder): results are bit-identical for every chunk size. */
int mxa_bed2compressed(const char *bed_path, int snps, int indiv, int max_n, void **compressed, double *f_out, int *snps_out,
                       int *indiv_out);

/* The same for SNP rows [snp_begin, snp_end) of the file only: ONLY those rows are read (fseek), the individual-major block and
 * the frequencies of the range are produced on the device, and the object behaves like one made by mxa_plink2compressed_shard --
 * without any process ever holding the full SNP-major or individual-major matrix (one-process-per-GPU jobs: every rank stages
 * its own range; the in-process sharder below does the same per device).  snps / indiv <= 0: from .bim / .fam.  f_out
 * (optional, host) receives the snp_end - snp_begin frequencies of the range.  Returns 0 / 1. */
int mxa_bed2compressed_range(const char *bed_path, int snps, int indiv, int snp_begin, int snp_end, int max_n, void **compressed,
                             double *f_out);

/* Incremental staging (round 5): plink2compressed (5codesAPI.c:80-96 -> plink2gpu, dgemm_compressed_cuda.cu:43-170) wants the whole PLINK matrix
 * behind one pointer and the reference gives up when matrix + object exceed the device (dgemm_compressed_cuda.cu:93-100).  Here the object is
 * allocated first -- ONE packed copy (a single-orientation object, see mxa_single_orientation below) -- and filled by blocks of SNP rows, so that
 * BASELINE config 4 at its full 5M x 200k (250 GB packed) is staged on one 288 GB device from a generator / reader that holds one block at a time.
 *   mxa_plink2compressed_begin: allocate (packed matrix zeroed; options as plink2compressed).  *compressed NULL on failure.
 *   mxa_plink2compressed_rows : SNP rows [snp_begin, snp_begin + nrows) = nrows compact PLINK rows of ceil(indiv/4) bytes, host or device memory;
 *                               blocks may arrive in any order and must cover every row once.  f_rows: the nrows allele frequencies of the block,
 *                               or NULL -- then they are counted on the device with mxa_allele_freq's rule.  Returns when the block buffer may be reused.
 *   mxa_plink2compressed_end  : seal; get_compressed_freq returns the frequencies.  Products are refused (error 19) before this call.
 * mxa_bed2compressed(_range) use the same path for single-orientation objects: the .bed is streamed into the object in 64 MB chunks.
 * Products whose split-K partial sums would not fit beside such an object run their K splits in groups with the running sum kept in C
 * (same pieces, same order of additions: bit-identical to the one-pass product).  Return 0 / 1. */
int mxa_plink2compressed_begin(long snps, long indiv, int max_n, void **compressed);
int mxa_plink2compressed_rows(void *compressed, const unsigned char *plink_rows, long snp_begin, long nrows, const double *f_rows);
int mxa_plink2compressed_end(void *compressed);

/* ---- several GPUs behind the reference ABI (single process).  With MIRACULIX_NUM_GPUS=G (> 1) in the environment,
 * plink2compressed and mxa_bed2compressed return ONE handle that owns G per-device objects over contiguous SNP blocks
 * (boundaries at multiples of 4; devices HIP_DEVICE/CUDA_DEVICE (default 0) + 0..G-1 modulo the visible device count -- more
 * shards than devices puts several blocks on one GPU).  dgemm_compressed / mxa_gram_matvec / get_compressed_freq /
 * free_compressed accept it unchanged: 'N' multiplies every block on its own device (one host thread per device, so host
 * operands travel over every GPU's own PCIe link side by side) and sum-reduces the indiv x n partials onto the first device --
 * by default with peer-to-peer pushes over xGMI and ONE addition kernel in ascending block order (bitwise reproducible),
 * with MXA_REDUCE=rccl by ncclReduce (RCCL is dlopen()ed; needs distinct devices); 'T' writes disjoint row blocks, no exchange.
 * B / C may be host memory or memory of any of the devices (work the caller enqueued on that device's default stream is waited for
 * first).  mxa_dgemm_compressed_device is not available on such a handle; mxa_dgemm_compressed_multi (below) takes per-device operand slices.
 * Peer access between the devices is enabled at creation and the verdicts are logged (PRINT_LEVEL > 0) and reported by mxa_multi_shard_info.
 * NOT YET MEASURED on more than one physical GPU: all of it runs in the tests with several shards on one device.
 * snp_multiply_gpu with host operands follows the same variable: device g computes the column panel [c_g, c_g+1) of the symmetric result (equal
 * numbers of 256-column tiles = equal work), staging the packed matrix itself, and downloads it over its own PCIe link into its slab of the host
 * matrix -- independent units, no exchange; bit-identical to the single-device result.
 * mxa_num_shards: number of per-device objects behind a handle (1 for an ordinary one).  mxa_shard_bounds: block g of the
 * partition of `snps` into `shards` blocks; returns the number of non-empty blocks. */
int mxa_num_shards(void *compressed);
int mxa_shard_bounds(long snps, int shards, int g, long *begin, long *end);

/* dgemm_compressed on a multi-device object with the operands handed over PER SHARD, so that nothing but the indiv x n partial sums
 * crosses a device boundary (with ONE B / C pointer, as through dgemm_compressed, the device that holds them is a hub: every shard
 * copies its slice from / to it).  Arrays of mxa_num_shards(compressed) pointers; block g = mxa_shard_bounds(snps, shards, g, ..):
 *   'N': B_per_shard[g] = rows [begin_g, end_g) of B (leading dimension ldb), normally memory of shard g's device;
 *        C_per_shard[0] receives the reduced indiv x n result (leading dimension ldc; memory of the first shard's device, of any other
 *        device, or of the host); the other entries of C_per_shard are ignored.
 *   'T': B_per_shard[g] = the whole indiv x n matrix B as shard g reads it (leading dimension ldb; a NULL entry g > 0 makes shard g read
 *        B_per_shard[0] across devices); C_per_shard[g] = rows [begin_g, end_g) of C (leading dimension ldc >= end_g - begin_g; rows
 *        beyond the block are not touched).
 * sync == 0: the call returns when the work is enqueued (device operands only; a host operand makes the call synchronous).  Products
 * issued back to back on one object are ordered like calls on one stream, but the transfers of an 'N' product's partial sums and their
 * addition on the first device run BESIDE the next product ('T' of the same step) on copy streams.  mxa_multi_synchronize() waits for
 * everything issued on the object (a later product that READS or overwrites the memory the previous 'N' product delivered its result to is
 * ordered behind that delivery; products on unrelated memory are not held up).  Results are those of dgemm_compressed on the same object (same
 * kernels, same fixed-order reduction).
 * Reference counterpart of the need: src/cuda/dgemm_compressed_cuda.cu:251-252 (operands cross PCIe on every call).  Returns 0 / 1. */
int mxa_dgemm_compressed_multi(char trans, void *compressed, int n, const double *const *B_per_shard, long ldb,
                               double *const *C_per_shard, long ldc, int sync);
int mxa_multi_synchronize(void *compressed);

/* reduction of the 'N' partial sums on a multi-device object: 0 = peer-to-peer pushes + ONE addition kernel in ascending shard order
 * (default; bitwise reproducible), 1 = RCCL ncclReduce (one rank per shard, all in this process; needs one device per shard).
 * Returns 0, 1 (error) or 2 (RCCL not applicable: several shards share a device; the reduction is unchanged).  The FIRST RCCL reduction of
 * an object is cross-checked: the same partial sums are also reduced peer-to-peer and the two results compared (<= 1e-13 of the largest
 * entry, else the product fails with error 18); mxa_multi_get_info reports the difference. */
int mxa_multi_set_reduction(void *compressed, int kind);

/* what a multi-device object is made of and what it has done since mxa_multi_reset_profile (HIP events on the streams the work ran on) */
typedef struct mxa_multi_info {
  int shards, devices, root_device;
  int reduction;                     /* 0 peer-to-peer fixed order, 1 RCCL */
  int reductions; double reduce_ms;  /* addition kernel on the root device (RCCL: the ld-padded copy of the received sum) */
  int rccl_checked; double rccl_vs_p2p_max_rel_diff;   /* -1 until an RCCL reduction has been cross-checked */
} mxa_multi_info;
typedef struct mxa_shard_info {
  int device; long snp_begin, snp_end;
  int peer_to_root, peer_from_root;          /* 1 peer access enabled (direct xGMI), 0 not available (copies are staged through the host), -1 same device */
  int kernel_launches; double kernel_ms;     /* dominant kernel of this shard's products */
  int in_copies; double in_ms;               /* operand distribution: copies of a B that did not live on this shard's device */
  int out_copies; double out_ms;             /* result gather: copies of a 'T' row block to a C that did not live on this shard's device */
  int pushes; double push_ms;                /* partial sums pushed to the root device (RCCL: shard 0 = the ncclReduce) */
} mxa_shard_info;
int mxa_multi_get_info(void *compressed, mxa_multi_info *out);
int mxa_multi_shard_info(void *compressed, int shard, mxa_shard_info *out);
int mxa_multi_reset_profile(void *compressed);

/* Output-tile sharding of the crossproduct for one-process-per-GPU use (packed matrix replicated, independent
 * units, no collective): columns [col_begin, col_end) of the symmetric result of snp_multiply_gpu, i.e. the contiguous slab
 * ans + col_begin*indiv of the full column-major matrix, into `panel` (indiv rows, col_end - col_begin columns, leading
 * dimension ld).  col_begin must be a multiple of 256, col_end a multiple of 256 or == indiv.  upper_only != 0 computes only
 * rows [0, col_end) of the panel, i.e. everything above its diagonal block and the block itself (a host panel gets zeros in the
 * rows below, a device panel is left untouched there) -- half the total work for callers that exchange the transposed blocks
 * (miraculix_amd/distributed.py: crossprod_sharded).  Same argument meaning otherwise as snp_multiply_gpu, padding bits included (AS STORED).  Returns 0 / 1. */
int mxa_snp_multiply_panel(const unsigned char *snp_matrix, int snps, int indiv, int col_begin, int col_end, int upper_only,
                           double *panel, long ld, int is_plink_format);

/* GRM and LD with the post-processing done on the device before the result leaves HBM (reference: host BLAS in
 * src/bindings/Julia/crossproduct.jl:83-110 grm(), :128-152 ld(); maths docs/grm.md:5-12).
 * mxa_grm: G(indiv x indiv) = P Z Z^T P^T [/ (2 sum f(1-f))], plink_transposed = indiv rows of ceil(snps/4) bytes.
 * mxa_ld : R(snps x snps)  = D^-1/2 (Z^T Z - 4 indiv f f^T) D^-1/2,  plink = snps rows of ceil(indiv/4) bytes.
 * Pointers may be host or device.  Return 0 / 1.
 * The element-wise map runs INSIDE the crossproduct epilogue (round 3): the column sums and the diagonal of the crossproduct are formed from
 * the packed matrix before the product (exact integers), so the result is written once and a host result leaves through the same slab
 * pipeline as snp_multiply_gpu's.  The reference's divisions (by 2 sum f(1-f); by sigma_i, sigma_j) are multiplications by reciprocals
 * (<= 1 ulp from the quotients).  MXA_XPROD_FUSED_POST=0 runs the three separate passes over the result instead (bit-identical).
 * Padding bits: IGNORED by mxa_grm, mxa_ld and every plain windowed entry below (mxa_ld_band, mxa_ld_scores, mxa_ld_window_rows / _scores / _pairs / _prune /
 * _apply, mxa_ld_op_create), unlike snp_multiply_gpu: the fields at and beyond the row's length are staged as 00 BEFORE the byte table, so they are no
 * individuals (mxa_ld; `indiv` and f in its formula do not count them either) and no SNPs (mxa_grm), and a padding 01 does not turn its byte into 3s. */
int mxa_grm(const unsigned char *plink_transposed, int snps, int indiv, double *G, int is_plink_format, int do_scale,
            const double *allele_freq);
int mxa_ld(const unsigned char *plink, int snps, int indiv, double *R, int is_plink_format, const double *allele_freq);

/* Windowed LD: the entries of mxa_ld's R within `window` SNPs of the diagonal, without the snps x snps matrix -- O(snps * window) work and memory, so
 * LD at 1 000 000 SNPs is one call.  Arguments as mxa_ld (plink = snps rows of ceil(indiv/4) bytes; every pointer host or device); window = number of
 * neighbours on each side, counted in SNPs, 0 <= window < snps.  A chromosome is a row range of the SNP-major matrix: a pointer offset and a smaller snps.
 * mxa_ld_band  : band[d + i*ldb] = R(i, i+d) for 0 <= d <= window, i + d < snps; 0.0 where i + d >= snps; rows d > window of a wider ldb (>= window + 1)
 *                are not touched.  This is LAPACK's lower symmetric band storage AB(1+i-j, j) = A(i, j) (dsbmv, dpbtrf).  kind 0: r, 1: r^2 (r*r, one rounding).
 * mxa_ld_scores: scores[i] = sum over j, |i-j| <= window (j = i included), of t(r_ij); adjust 0: t = r^2, 1: t = r^2 - (1 - r^2) / (indiv - 2), formed as
 *                r2 - (1 - r2) * (1 / (indiv - 2)) with every operation rounded (needs indiv >= 3).  The band is never written to memory.
 * R is mxa_ld's R bit for bit (same staging, byte table, statistics and map), from the same two exact engines; the scores are sums in a fixed order
 * (no atomics): identical from run to run and between the engines.  A monomorphic SNP has sigma = 0: its entries are non-finite exactly as mxa_ld's
 * are, and a score whose window holds such an entry is non-finite -- no special case; filter such SNPs before the call.
 * Errors (return 1, mxa_last_error() == 1, output untouched): window out of range, ldb < window + 1, kind / adjust not 0 or 1, adjust with indiv < 3,
 * allele_freq == NULL, snps >= 29 000 000; 12: not enough device memory.  Runs on the selected device (no MIRACULIX_NUM_GPUS sharding). */
int mxa_ld_band(const unsigned char *plink, int snps, int indiv, int window, double *band, long ldb, int kind, int is_plink_format,
                const double *allele_freq);
int mxa_ld_scores(const unsigned char *plink, int snps, int indiv, int window, double *scores, int adjust, int is_plink_format,
                  const double *allele_freq);

/* Windowed LD on data WITH missing genotypes: the pairwise-complete correlation (what PLINK's --r / --r2 report).  mxa_ld_band / mxa_ld_scores stage the
 * matrix with the reference's byte table, under which a byte that holds a missing pair (01) becomes four 3s: their results on such data are not correlations.
 * Here, for SNP rows i, j of the PLINK matrix, with m = 1 where the genotype is present (0 for the missing code 01), z = the allele count with missing as 0
 * and a = 1 where the code is 11 (so z^2 = z + 2 a), all sums over the `indiv` individuals of a row:
 *     N   = sum m_i m_j           Sxy = sum z_i z_j           Sx = sum z_i m_j           Sy = sum m_i z_j
 *     Sxx = Sx + 2 sum a_i m_j    Syy = Sy + 2 sum m_i a_j
 *     num = N Sxy - Sx Sy         dx  = N Sxx - Sx^2          dy = N Syy - Sy^2          r = num / sqrt(dx * dy)
 * i.e. Pearson's r over the individuals genotyped at BOTH SNPs.  The six sums are exact integer tile products (the crossproduct engines); num, dx, dy are
 * formed exactly (integers below 4 indiv^2 < 2^53); then ONE product dx * dy, ONE square root and ONE quotient, each correctly rounded, in that order.
 * A pair with dx * dy = 0 -- no individual genotyped at both SNPs, or a SNP constant on the shared ones -- gives 0 / 0 = NaN: no special case (as a
 * monomorphic SNP in mxa_ld).  r is symmetric in (i, j) bit for bit.
 * plink: snps rows of ceil(indiv / 4) bytes in PLINK coding (00 -> 0, 01 -> missing, 10 -> 1, 11 -> 2; there is no raw 2-bit form: only PLINK coding has a
 * missing code), host or device.  The padding bits of a row's last byte (fields at and beyond indiv) are NOT individuals, whatever they hold.  No
 * allele_freq: every statistic comes from the data.
 * mxa_ld_band_pairwise  : band layout, window, ldb, kind (0: r, 1: r * r, one rounding), zeros in the tail, rows beyond window of a wider ldb untouched:
 *                         exactly as mxa_ld_band.
 * mxa_ld_scores_pairwise: scores[i] = sum over j, |i-j| <= window (j = i included), of t(r_ij); adjust 0: t = r^2; 1: t = r^2 - (1 - r^2) / (N_ij - 2) with the
 *                         pair's own N_ij, formed as r2 - ((1 - r2) / (N - 2)) with every operation rounded on its own.  Fixed summation order, no atomics.
 *                         The r inside a term is bit for bit the r mxa_ld_band_pairwise returns for that pair.
 * Results are identical from run to run, between the FP4 and the int8 engine (MXA_XPROD_ENGINE=i8), between host and device pointers, and for every size of
 * the count scratch: the band runs in groups of tile rows whose six int32 count tiles per 256 x 256 band tile stay under MXA_LD_PAIRWISE_SCRATCH_MB (default
 * 2048; one tile row at least).  A matrix without any missing code needs the sum z_i z_j product only (N = indiv, the rest are per-SNP sums): same bits,
 * about the cost of mxa_ld_band; MXA_LD_PAIRWISE_DENSE=1 forces the six products.  Device memory: three 2-bit planes of the matrix (3 x mxa_ld_band's).
 * Errors (return 1, mxa_last_error() == 1, output untouched): window out of range, ldb < window + 1, kind / adjust not 0 or 1, adjust with indiv < 3,
 * indiv > 47 453 132 (4 indiv^2 >= 2^53), snps >= 29 000 000; 12: not enough device memory.  Runs on the selected device (no MIRACULIX_NUM_GPUS sharding). */
int mxa_ld_band_pairwise(const unsigned char *plink, int snps, int indiv, int window, double *band, long ldb, int kind);
int mxa_ld_scores_pairwise(const unsigned char *plink, int snps, int indiv, int window, double *scores, int adjust);

/* Windowed LD by distance: windows in base pairs or centimorgans that stop at chromosome ends, for a whole genome in one call.  The window is data: an array
 * `last` of snps ints with i <= last[i] < snps and last[i] <= last[i+1]; SNP j >= i is in the window of i iff j <= last[i].  The relation is symmetric by
 * construction (the score of j counts i < j iff j <= last[i]) and covers bp, cM and SNP-count windows and chromosome breaks alike.
 *
 * mxa_ld_window_bounds (host only, no device needed; O(snps), a two-pointer sweep): last[i] = the largest j >= i with chrom[j] == chrom[i],
 *   pos[j] - pos[i] <= max_dist (ONE rounded fp64 subtraction, inclusive comparison) and j - i <= max_snps.  chrom == NULL: one chromosome; pos == NULL: no
 *   distance bound (max_snps >= 0 is then required); max_snps < 0: no SNP bound.  rowptr (optional, snps + 1 longs): the exclusive prefix sum of
 *   last[i] - i + 1, so rowptr[snps] is the number of entries mxa_ld_window_rows stores.  Returns 1 (mxa_last_error() == 1, outputs untouched) for snps <= 0,
 *   last == NULL, max_dist negative or NaN, a NaN position, a position that decreases inside a chromosome, a chromosome code that returns after another one
 *   (chromosomes must be contiguous), neither bound given.
 *
 * The four device entries take `last` (host or device pointer, like every pointer here; it is copied to the host, checked, and the tile plan made from it):
 * mxa_ld_window_rows  : ragged rows, rows[rowptr[i] + d] = R(i, i + d) for 0 <= d <= last[i] - i, rowptr as above (formed by the entry; the caller allocates
 *                       rowptr[snps] doubles).  No zero fill, no leading dimension, nothing written beyond rowptr[snps]: a dense region with a reach of 20 000
 *                       SNPs costs its own rows only.  kind 0: r, 1: r * r (one rounding).
 * mxa_ld_window_scores: scores[i] = sum of t(r_ij) over first[i] <= j <= last[i], first[i] = min{k : last[k] >= i}; t and adjust as mxa_ld_scores.
 * mxa_ld_window_rows_pairwise, mxa_ld_window_scores_pairwise: the same from the pairwise-complete r of mxa_ld_band_pairwise (per-pair N_ij in the adjusted
 *                       term; MXA_LD_PAIRWISE_SCRATCH_MB bounds the count scratch of a group of consecutive tile rows, one tile row at least; the results do
 *                       not depend on it; the missing-free shortcut and MXA_LD_PAIRWISE_DENSE as there).
 * R, the terms, kind, adjust and the NaN behaviour are those of the fixed entries: the same kernels, engines, map and store, with the window read from
 * last[] instead of one number.  Tile row I holds the 256 x 256 tiles (I, J), I <= J <= last[min(256 I + 255, snps - 1)] / 256.  With
 * last[i] = min(i + w, snps - 1) this is the tile set and the summation order of the fixed entries: rows and scores are the same bits as theirs.
 * Errors (return 1, mxa_last_error() == 1, output untouched): NULL pointers, last out of range or decreasing, kind / adjust not 0 or 1, adjust with
 * indiv < 3, the fixed entries' snps and indiv bounds, allele_freq == NULL on the plain route; 12: not enough device memory (last, rowptr and the scores'
 * partial buffer are counted).  Runs on the selected device (no MIRACULIX_NUM_GPUS sharding). */
int mxa_ld_window_bounds(int snps, const double *pos, const int *chrom, double max_dist, int max_snps, int *last, long *rowptr);
int mxa_ld_window_rows(const unsigned char *plink, int snps, int indiv, const int *last, double *rows, int kind, int is_plink_format,
                       const double *allele_freq);
int mxa_ld_window_scores(const unsigned char *plink, int snps, int indiv, const int *last, double *scores, int adjust, int is_plink_format,
                         const double *allele_freq);
int mxa_ld_window_rows_pairwise(const unsigned char *plink, int snps, int indiv, const int *last, double *rows, int kind);
int mxa_ld_window_scores_pairwise(const unsigned char *plink, int snps, int indiv, const int *last, double *scores, int adjust);

/* The pairs of a window with r^2 at or above a cutoff, as a sparse list compacted on the device (what PLINK's --r2 --ld-window-kb .. --ld-window-r2 gives): the
 * fourth output form of the general window, next to band, ragged rows and scores.  The rows never exist; the result costs its own pairs only.
 * plink, snps, indiv, last, is_plink_format, allele_freq: exactly as for mxa_ld_window_rows / mxa_ld_window_rows_pairwise (same staging, byte table,
 * statistics, engines and bounds).  A fixed window of w SNPs is last[i] = min(i + w, snps - 1).
 * Candidates: the pairs (i, j), i < j <= last[i] (the diagonal is not a pair).  With r^ = bit for bit the value mxa_ld_window_rows(_pairwise) stores for the
 * pair at kind 0, and q = fl(r^ * r^) (one rounding: the kind-1 value), the pair is kept iff q >= min_r2.  A NaN r^ is never kept (the comparison is false): a
 * monomorphic SNP on the plain route, a pair with dx * dy = 0 on the pairwise route; no special case.
 * Result, CSR of the strict upper triangle: rowptr (snps + 1 longs, rowptr[0] = 0); the kept pairs of row i at rowptr[i] .. rowptr[i + 1] - 1, col strictly
 * ascending; val = r^ (kind 0) or q (kind 1); *total = rowptr[snps] (total: a host pointer, required).
 * Count-only call (col == NULL and val == NULL): rowptr and *total are written, capacity is ignored, returns 0.
 * Filling call (col and val given, `capacity` entries each): nothing at or beyond capacity is written.  total <= capacity: returns 0, nothing at or beyond
 * total is written.  total > capacity: returns 1 with mxa_last_error() == 25; rowptr and *total are valid (the message names both numbers), the contents of
 * col / val are unspecified.
 * rowptr, col, val: all host or all device pointers; plink, last, allele_freq host or device independently.
 * The window's tile products run once, into int32 count tiles of 256 KiB in groups of tile rows under MXA_LD_PAIRWISE_SCRATCH_MB (as the pairwise entries:
 * six per window tile, or one on data without a missing code; one on the plain route); per group a count pass, a scan and a write pass.  Every position is a
 * sum of counts in a fixed order (no atomics): rowptr, col and val are identical from run to run, between the FP4 and the int8 engine (MXA_XPROD_ENGINE=i8),
 * between host and device pointers, and for every scratch size.
 * Errors (return 1, mxa_last_error() == 1, outputs untouched): everything mxa_ld_window_rows(_pairwise) rejects; rowptr == NULL or total == NULL; exactly one
 * of col / val NULL; capacity < 0 on a filling call; min_r2 negative, NaN or infinite (min_r2 > 1 is legal: the result is normally empty); kind not 0 or 1;
 * rowptr, col, val not all host or all device.  12: not enough device memory (the scratch, the per-(tile, row) counters and, for host outputs, the device
 * copies of rowptr / col / val are counted). */
int mxa_ld_window_pairs(const unsigned char *plink, int snps, int indiv, const int *last, double min_r2, int kind, long *rowptr, int *col, double *val,
                        long capacity, long *total, int is_plink_format, const double *allele_freq);
int mxa_ld_window_pairs_pairwise(const unsigned char *plink, int snps, int indiv, const int *last, double min_r2, int kind, long *rowptr, int *col,
                                 double *val, long capacity, long *total);

/* LD pruning and clumping: the greedy selection on the pairs graph, on the device (what PLINK's --indep-pairwise / --clump and bigsnpr's snp_clumping ask for:
 * a subset of SNPs in which no two within the window are in LD above a threshold, chosen in priority order).
 * G is the graph on the SNPs 0 .. snps - 1 whose edges are exactly the pairs mxa_ld_window_pairs(_pairwise) keeps for the same plink, last, min_r2 and route:
 * i < j <= last[i], q = fl(r^ * r^) >= min_r2, a NaN r^ is never an edge.  SNP a comes before SNP b iff priority[a] < priority[b], or the priorities are equal
 * and a < b; priority == NULL: iff a < b.  Smaller goes first: p-values for clumping, -MAF for pruning.  Result: walk the SNPs in that order and keep a SNP iff
 * none of its neighbours in G has been kept.  This is the lexicographically first maximal independent set of G under the order; it is unique, so keep, owner,
 * *n_kept and *rounds do not depend on the engine, the pointer kinds, the scratch size or any schedule.
 * keep: snps bytes of 0 / 1.  owner (optional, NULL skips its pass): snps ints, owner[v] = v for a kept v, else the first kept neighbour of v in the order -- the
 * SNP that removes v in the walk, PLINK's index SNP of v's clump.  keep and owner: both host or both device pointers.  n_kept: a host pointer, required.
 * rounds (optional, a host pointer): the number of rounds the device ran = the length of the longest dependency chain; small for priorities unrelated to
 * position (p-values, MAF), about snps for priority == NULL on a long run of mutual LD (a path in index order takes snps rounds), each round two launches and
 * one sweep over the rows.  *rounds <= snps always.
 * mxa_ld_prune_csr: the graph step alone on any CSR of the strict upper triangle, e.g. the one mxa_ld_window_pairs returned (one pair list, several
 * priorities, no second product).  rowptr (snps + 1 longs), col, priority: host or device pointers, each independently; col may be NULL when rowptr[snps] == 0.
 * The CSR is checked where it lies (host loop, or a checking kernel whose flag the host reads): rowptr[0] == 0, rowptr non-decreasing, in every row
 * i < col < snps strictly ascending.
 * mxa_ld_window_prune(_pairwise): the pairs driver and the graph step; neither the pair list nor a val array leaves the device or is ever formed for the host.
 * A count-only pass sizes col exactly, a filling pass writes col alone: the window's products run twice, as in the count-then-fill use of mxa_ld_window_pairs.
 * snps == 1 is legal: keep = {1}, owner = {0}.
 * Errors (return 1, mxa_last_error() == 1, outputs untouched): keep or n_kept NULL; keep / owner not both host or both device; a NaN in priority (+-inf is
 * legal); mxa_ld_prune_csr: snps <= 0, rowptr NULL, a CSR that fails the check; the window entries: everything mxa_ld_window_pairs(_pairwise) rejects for these
 * arguments.  12: not enough device memory (col, rowptr, the per-SNP state and owner arrays, and the scratch as the pairs entries count it). */
int mxa_ld_prune_csr(int snps, const long *rowptr, const int *col, const double *priority, unsigned char *keep, int *owner, long *n_kept, int *rounds);
int mxa_ld_window_prune(const unsigned char *plink, int snps, int indiv, const int *last, double min_r2, const double *priority, unsigned char *keep, int *owner,
                        long *n_kept, int *rounds, int is_plink_format, const double *allele_freq);
int mxa_ld_window_prune_pairwise(const unsigned char *plink, int snps, int indiv, const int *last, double min_r2, const double *priority, unsigned char *keep,
                                 int *owner, long *n_kept, int *rounds);

/* The window applied to a matrix: Y = T_w(R) X without the rows.  Y[i, c] = sum over first[i] <= j <= last[i] of t(r_ij) X[j, c], first[i] = min{k: last[k] >= i}
 * as in mxa_ld_window_scores; for j < i the value is that of the pair (j, i), the diagonal is one term, counted once.  mxa_ld_window_scores is this product
 * with n = 1, X = 1.  Uses: partitioned (stratified) LD scores l(i, c) = sum_j r2_ij a_jc for an annotation matrix a (ldsc --l2 --annot), MAF-binned or
 * weighted scores (indicator or weight columns), and R_w X with t = r for summary-statistics methods (one call per product of a conjugate-gradient solve).
 * plink, snps, indiv, last, is_plink_format, allele_freq: exactly as for mxa_ld_window_rows / mxa_ld_window_rows_pairwise (staging, byte table, statistics,
 * engines, bounds, the missing-free shortcut); a fixed window is last[i] = min(i + w, snps - 1).
 * X: snps x n, column-major, ldx >= snps; Y: snps x n, column-major, ldy >= snps (dgemm_compressed's B / C).  X and Y are each a host or a device pointer,
 * independently.  Rows snps .. ldy - 1 of a column of Y are never written, nor is anything beyond column n - 1.
 * term: 0: t = r^; 1: t = fl(r^ r^); 2: the adjusted term of the scores entries -- plain route r2 - (1 - r2) (1 / (indiv - 2)), pairwise route
 * r2 - ((1 - r2) / (N_ij - 2)) with the pair's own N_ij.  r^ is bit for bit the value mxa_ld_window_rows(_pairwise) stores for the pair at kind 0.
 * NaN: a monomorphic SNP (plain route) or a pair with dx dy = 0 (pairwise route) makes its term NaN, and every Y[i, .] whose window holds it is then NaN, even
 * where X[j, c] = 0: filter such SNPs before the call.  (An element outside the window is skipped, never multiplied: X may hold anything there.)
 * Every Y[i, c] is a sum in a fixed order, no floating-point atomics: Y is identical from run to run, between the FP4 and the int8 engine
 * (MXA_XPROD_ENGINE=i8), between host and device pointers, for every MXA_LD_PAIRWISE_SCRATCH_MB, and for every n: column c of an n-column call is bit for
 * bit the one-column call on that column.  The window's tile products run once, into the int32 count tiles of the pairs entries; per window tile
 * 4 KiB n of partial sums share the scratch cap with them.
 * Errors (return 1, mxa_last_error() == 1, Y untouched): everything mxa_ld_window_rows(_pairwise) rejects; X or Y NULL; n < 1 (or n > 1 048 560); ldx < snps
 * or ldy < snps; term not 0, 1 or 2; term == 2 with indiv < 3.  12: not enough device memory (the scratch, the partial sums and the device copies of a host
 * X / Y are counted). */
int mxa_ld_window_apply(const unsigned char *plink, int snps, int indiv, const int *last, int term, const double *X, long ldx, int n, double *Y, long ldy,
                        int is_plink_format, const double *allele_freq);
int mxa_ld_window_apply_pairwise(const unsigned char *plink, int snps, int indiv, const int *last, int term, const double *X, long ldx, int n, double *Y,
                                 long ldy);

/* The LD operator object: the window's values staged ONCE in device memory, then applied and ridge-solved there.  mxa_ld_window_apply forms every r^ anew on
 * each call; LDpred-inf, SBLUP and ridge regression on summary statistics apply the same T_w(R) tens to hundreds of times.  The object holds
 * T[i, j] for first[i] <= j <= last[i] (first[i] = min{k : last[k] >= i}), symmetric; kind 0: T = r^, kind 1: T = fl(r^ r^) -- bit for bit what
 * mxa_ld_window_rows / mxa_ld_window_rows_pairwise store for the same arguments: creation runs that driver into a device buffer.  The adjusted term (term 2 of
 * mxa_ld_window_apply) is not offered.  The object lives in the memory of the selected device (no MIRACULIX_NUM_GPUS sharding); one call is in flight per
 * object, as for the compressed objects.
 * Storage: the MIRRORED ragged rows in one array, row j = T[j, first[j] .. last[j]] at ptr[j] (ptr = exclusive prefix sum of last[j] - first[j] + 1), i.e.
 * 2 entries - snps doubles with entries = rowptr[snps], the number of upper entries; first, last, ptr, rowptr, ptr - first and a packing buffer of 16 doubles
 * per SNP (the column chunk of an apply) sit beside it.  Peak during creation: the upper rows (8 entries bytes, released at the end) plus the larger of the
 * object (`bytes`) and the rows driver's own staging.
 * mxa_ld_op_bytes (host only, no device needed; last: a host pointer): *entries and *bytes (what an object holds after creation) from `last` alone.
 * mxa_ld_op_create / _create_pairwise: arguments as mxa_ld_window_rows / mxa_ld_window_rows_pairwise; *op receives the handle.
 * mxa_ld_op_from_rows: the same object from caller-supplied upper ragged rows (mxa_ld_window_rows' layout, `entries` doubles, host or device; copied): LD from
 *   another source.  The values are taken as they are (no unit diagonal is required).
 * mxa_ld_op_rows: the upper ragged rows back out, `entries` doubles, host or device.
 * mxa_ld_op_apply: Y[i, c] = shift X[i, c] + sum over first[i] <= j <= last[i] of T[i, j] X[j, c].  X, Y: snps x n column-major, ldx, ldy >= snps, each a host
 *   or a device pointer independently; rows snps .. ldy - 1 of Y and anything beyond column n - 1 are never written; X and Y must not overlap.  The sum is the
 *   chain acc = fma(T[i, j], X[j, c], acc) over ascending j from 0.0, then fma(shift, X[i, c], acc): an order fixed by i and the window alone, no atomics.  Y
 *   is identical from run to run, between host and device pointers and for every n (column c of an n-column call is bit for bit the one-column call).  An
 *   element outside the window is skipped, never multiplied; a NaN in T makes exactly the rows whose window holds it NaN.
 * mxa_ld_op_solve: (T + shift I) X = B by conjugate gradients from X = 0, the n columns in lockstep, each with its own alpha, beta, iteration count and
 *   stopping decision, all kept on the device (the host reads one word per iteration: the number of columns still running).  A column stops when the
 *   recurrence residual satisfies sqrt(r.r) / sqrt(b.b) <= tol, tested before the first iteration too (b = 0: X = 0, iters 0).  status[c]: 0 converged, 1
 *   max_iter reached, 2 breakdown (p.Ap not > 0: the matrix is not positive definite along p, or a NaN); after 1 or 2, X holds the last iterate.  relres[c]:
 *   the final recurrence residual over the norm of b (0 for b = 0); iters, relres, status: optional host arrays of n.  Dot products are per-block partials
 *   (1024 rows each) summed by one block in index order: column c of an n-column solve, its iters included, is bit for bit the one-column solve.  The return
 *   value is 0 whenever the call ran; the verdict is per column.  B, X: host or device independently, must not overlap.
 * mxa_ld_op_free: releases the object and sets *op = NULL; NULL or an already freed handle: no-op.
 * Errors (return 1, mxa_last_error() == 1, outputs untouched, *op left NULL on creation): everything mxa_ld_window_rows(_pairwise) rejects; NULL op or pointers;
 * n < 1 (solve: n > 65535); ldx / ldy / ldb < snps; overlap of X and Y (B and X) between pointers of the same kind; shift NaN or infinite; tol not in (0, 1); max_iter < 0; a
 * handle that is not live.  12: not enough device memory (creation: upper rows plus object; apply: the device copies of host X / Y; solve: r, p, Ap, the
 * partial sums and the device copies of host B / X). */
int mxa_ld_op_bytes(int snps, const int *last, long *entries, long *bytes);
int mxa_ld_op_create(const unsigned char *plink, int snps, int indiv, const int *last, int kind, int is_plink_format, const double *allele_freq, void **op);
int mxa_ld_op_create_pairwise(const unsigned char *plink, int snps, int indiv, const int *last, int kind, void **op);
int mxa_ld_op_from_rows(int snps, const int *last, const double *rows, void **op);
int mxa_ld_op_rows(void *op, double *rows);
int mxa_ld_op_apply(void *op, double shift, const double *X, long ldx, int n, double *Y, long ldy);
int mxa_ld_op_solve(void *op, double shift, const double *B, long ldb, int n, double *X, long ldx, double tol, int max_iter, int *iters, double *relres,
                    int *status);
void mxa_ld_op_free(void **op);

/* Association scan: per-SNP linear regression on packed genotypes -- the statistics the LD entries above start from.  For every SNP s and phenotype c the
 * model y_c ~ 1 + Q + x_s, x_s = the genotype with missing calls replaced by the SNP's mean over its called individuals (what BOLT, fastGWA and regenie do).
 * plink: snps rows of ceil(indiv / 4) bytes in PLINK coding (00 -> 0, 01 -> missing, 10 -> 1, 11 -> 2), host or device.  The padding fields of a row's last
 *        byte (fields at and beyond indiv) are NOT individuals, whatever they hold.
 * Y:     indiv x n phenotypes, column-major, ldy >= indiv.  Q: indiv x k covariate basis, column-major, ldq >= indiv, k >= 0; NULL iff k == 0.  Q is taken
 *        as it is: its columns are expected to be orthonormal and to sum to zero -- exactly what mxa_assoc_basis produces.  An intercept is always fitted.
 * Degrees of freedom: dof = indiv - k - 2 >= 1.
 * Phenotypes, once per call, on the device: ybar_c = the column mean, y <- y - ybar_c; twice (the second pass for stability): a = Q^T y, y <- y - Q a; the
 * result is Y~; syy_c = sum y~^2; T_b = sum_i b_i for every column b of B = [Y~ | Q].  The summation orders of these steps are fixed by indiv and k alone,
 * no atomics; they are not otherwise specified.
 * Per SNP, exact integers from popcounts of the raw row (c1, c2 = the numbers of codes 10 and 11): N = the called individuals, Sz = c1 + 2 c2,
 * Szz = c1 + 4 c2.  Per SNP and column b of B: D_b = sum_i z_i b_i (z = the allele count, missing as 0: the library's own uncentred 'T' product on a one-shot
 * packed object, whatever setOptions_compressed said) and M_b = sum over the SNP's missing individuals of b_i, in a fixed order that depends on indiv alone,
 * no atomics.  Then, every operation rounded once, in this order:
 *     mu   = Sz / N
 *     v0   = (N Szz - Sz Sz) / N           numerator exact (integers below 4 indiv^2 < 2^53)
 *     g_b  = fma(mu, M_b - T_b, D_b)       for every column b of [Y~ | Q]
 *     sxx  = v0;  for q = 0 .. k-1 ascending: sxx = fma(-g_q, g_q, sxx)      (g_q: the Q columns)
 *     beta = g_c / sxx                     (g_c: the column of Y~)
 *     rss  = fma(-beta, g_c, syy_c)
 *     se   = sqrt((rss / dof) / sxx)
 *     t    = beta / se
 * There is no special case: N == 0, a SNP constant on its called individuals and a SNP in the span of [1, Q] give non-finite results where the arithmetic
 * says so; callers filter such SNPs, as for a monomorphic SNP in mxa_ld.  p-values are a wrapper's business (-|t| orders a clump).
 * Results are identical from run to run, between host and device pointers and for every row-chunk size of the staging (a host matrix is staged in chunks of
 * SNP rows, 256 MiB or MXA_ASSOC_CHUNK_ROWS rows each: each chunk is scanned, then appended to the packed object, so the raw matrix is never resident as a
 * whole).  They are NOT promised bit-identical between different n (or k): the product's narrow-n routes use different arithmetic.
 * mxa_assoc_basis (host only, no device needed): centres the q columns of W (indiv x q, ldw >= indiv), orthonormalises them in place order by Gram-Schmidt
 *   applied twice and writes Q (indiv x q, ldq >= indiv).  Errors (return 1, mxa_last_error() == 1, Q untouched): NULL pointers, indiv < 1, q < 0, ldw or ldq
 *   below indiv, a non-finite entry, a column whose norm after the two passes is at most indiv 2^-52 times its centred norm (constant or dependent; the
 *   message names it).
 * mxa_assoc_linear: beta, se, tstat: snps x n column-major, ldo >= snps; each optional, at least one required, those given all host or all device pointers;
 *   nothing is written beyond row snps - 1 of a column or beyond column n - 1.  nobs (optional, snps ints, host or device) receives N; dof (optional, host)
 *   receives indiv - k - 2.  plink, Y and Q are host or device pointers, each independently.  Errors (return 1, mxa_last_error() == 1, outputs untouched, all
 *   decided before a device is selected): NULL plink or Y; snps, indiv or n below 1; k < 0; n + k > 65535; Q == NULL with k > 0; a leading dimension too small;
 *   indiv - k - 2 < 1; indiv > 47 453 132; all three result pointers NULL; mixed host and device result pointers.  12: not enough device memory (the packed
 *   object, the staging chunk, B and its row-packed copy, the snps x (n + k) arrays D and M, device copies of host operands).  Runs on the selected device (no
 *   MIRACULIX_NUM_GPUS sharding). */
int mxa_assoc_basis(int indiv, const double *W, long ldw, int q, double *Q, long ldq);
int mxa_assoc_linear(const unsigned char *plink, int snps, int indiv, const double *Y, long ldy, int n, const double *Q, long ldq, int k, double *beta, double *se,
                     double *tstat, long ldo, int *nobs, int *dof);

/* Association scan for binary traits: the score test of a generalized linear null model on packed genotypes.  The null model is fitted ONCE per trait
 * (mxa_assoc_logistic_null for logistic regression; any other GLM null may be supplied by the caller); the scan then needs per SNP only inner products of the
 * genotype with fixed columns.  plink, the PLINK coding, the padding fields and x_s (missing calls replaced by mu = Sz / N) are those of mxa_assoc_linear.
 * Per trait c = 0 .. n-1 the caller supplies: the null residual r_c = column c of R (indiv x n, ldr >= indiv); the working weight w_c = column c of Wt
 * (indiv x n, ldw >= indiv); kh >= 0 projection columns h_{c,0..kh-1} = the columns c kh .. c kh + kh - 1 of H (indiv x n kh, ldh >= indiv; NULL iff kh == 0),
 * built so that sum_j (h_{c,j}^T x)^2 = x^T W C (C^T W C)^-1 C^T W x for the null design C and W = diag(w_c).  All column-major.
 * Per SNP, exact integers from popcounts of the raw row: N, c1, c2, Sz = c1 + 2 c2.  Per SNP and column b of B = [R | Wt | H] (n (kh + 2) columns):
 * D_b = sum_i z_i b_i (z = the allele count, missing as 0: the library's uncentred 'T' product on a one-shot packed object, whatever setOptions_compressed
 * said) and M_b = sum over the SNP's missing individuals of b_i.  Per SNP and weight column c: E_c = sum over the individuals with code 11 of w_{c,i}.  E_c and
 * M_b are summed in an order fixed by indiv (and kh, n) alone, no atomics.  Then, every operation rounded once, in this order:
 *     mu  = Sz / N
 *     U   = fma(mu, M_r, D_r)
 *     s2  = fma(2.0, E_c, D_w)                 (sum w z^2 = sum w z + 2 sum_{z = 2} w)
 *     m2  = mu * mu
 *     sxx = fma(m2, M_w, s2)
 *     for j = 0 .. kh-1 ascending:  a = fma(mu, M_hj, D_hj);  sxx = fma(-a, a, sxx)
 *     V   = sxx
 *     z   = U / sqrt(V)
 * score = U, var = V, zstat = z.  There is no special case: N == 0, V <= 0 and monomorphic SNPs give what the arithmetic gives; callers filter such SNPs.
 * No p-values here (-|z| orders a clump): saddlepoint p-values are mxa_assoc_score_spa, effect sizes by Firth-penalised fits mxa_assoc_score_firth.  Results are identical from run to run, between host and
 * device pointers and for every row-chunk size of the staging (MXA_ASSOC_CHUNK_ROWS applies as for mxa_assoc_linear); they are NOT promised bit-identical
 * between different column counts n (kh + 2).
 * mxa_assoc_score: score, var, zstat: snps x n column-major, ldo >= snps; each optional, at least one required, those given all host or all device pointers;
 *   nothing is written beyond row snps - 1 of a column or beyond column n - 1.  nobs (optional, snps ints, host or device) receives N.  plink, R, Wt and H are
 *   host or device pointers, each independently.  Errors (return 1, mxa_last_error() == 1, outputs untouched, all decided before a device is selected): NULL
 *   plink, R or Wt; snps, indiv or n below 1; kh < 0; H == NULL with kh > 0; n (kh + 2) > 65535; a leading dimension below its extent; indiv > 47 453 132; all
 *   three result pointers NULL; mixed host and device result pointers.  12: not enough device memory (what mxa_assoc_linear lists, and the snps x n array E).
 *   Runs on the selected device.
 * mxa_assoc_logistic_null (host only, no device needed): fits logit P(y_i = 1) = (C gamma)_i, C = [1 | W], W indiv x q (ldw >= indiv; NULL iff q == 0), y
 *   exactly 0 or 1, by Newton / IRLS: start at the intercept logit(ybar) and zeros; each step solves C^T W C delta = C^T (y - p) by Cholesky and is halved while
 *   the deviance rises (by more than 2^-50 of itself, the rounding of the sum; at most 20 halvings); stop when max_j |delta_j| <= tol max(1, max_j |gamma_j|).
 *   Sums are carried in long double.  Outputs: gamma (q + 1), r = y - p^, w = p^ (1 - p^) (indiv each), H (indiv x (q + 1), ldh >= indiv) = diag(w) C L^-T with L
 *   the lower Cholesky factor of C^T diag(w) C -- so kh = q + 1, H^T x = L^-1 C^T W x, and C^T H = L; iters (optional) = the Newton steps taken.  Errors (return
 *   1, mxa_last_error() == 1, outputs untouched, the message names the cause and the column): NULL pointers; indiv < 1, q < 0, indiv <= q + 1; a leading dimension
 *   below indiv; a y that is not exactly 0 or 1; all y equal; a non-finite covariate; C^T diag(w) C not positive definite (a pivot at most indiv 2^-52 times its
 *   diagonal entry: a constant or dependent column); no convergence within max_iter steps (separation).  12: not enough host memory for the work arrays (outputs
 *   untouched). */
int mxa_assoc_score(const unsigned char *plink, int snps, int indiv, const double *R, long ldr, const double *Wt, long ldw, const double *H, long ldh, int n, int kh,
                    double *score, double *var, double *zstat, long ldo, int *nobs);
int mxa_assoc_logistic_null(int indiv, const double *y, const double *W, long ldw, int q, double tol, int max_iter, double *gamma, double *r, double *w, double *H,
                            long ldh, int *iters);

/* The score test with saddlepoint p-values: mxa_assoc_score unchanged, then every (SNP s, trait c) with |z| >= z_cutoff is corrected on the device.  The
 * normal p-value erfc(|z| / sqrt 2) of the score test is badly anti-conservative for rare cases and rare alleles; the saddlepoint one needs, per SNP and
 * trait, a root solve over sums of a transcendental function of the covariate-adjusted genotype of all individuals, which no wrapper can form without the rows.
 * plink, R, Wt, H, n, kh, score, var, zstat and nobs are those of mxa_assoc_score, and score, var, zstat and nobs receive bit for bit what mxa_assoc_score
 * returns for the same operands.  P (indiv x n, ldp >= indiv, column-major): the null model's fitted probabilities p_{c,i}, expected in (0, 1) (for
 * mxa_assoc_logistic_null: p = y - r); Wt is expected to be positive.  Per (s, c), with mu, U, V, z and a_j = fma(mu, M_hj, D_hj) of mxa_assoc_score's chain,
 * x_i the allele count (missing calls: mu; padding fields are not individuals):
 *   flag 3  z is not finite: pval = NaN.
 *   flag 0  |z| < z_cutoff: pval = erfc(|z| sqrt(1/2)).
 *   else    tau_ij = h_{c,j,i} / w_{c,i};  g_i = x_i, then for j ascending g_i = fma(-a_j, tau_ij, g_i)   (for mxa_assoc_logistic_null's H this is
 *           x - C (C^T W C)^-1 C^T W x);  c0 = sum g_i p_i, A = sum |g_i|, G+ = sum max(g_i, 0), G- = sum min(g_i, 0).  The centred cumulant generating function
 *           of sum g_i y_i, y_i ~ Bernoulli(p_i), in an overflow-free form: with x = t g_i, e = exp(-|x|), (al, be) = (p_i, 1 - p_i) if x >= 0 else
 *           (1 - p_i, p_i), d = al + be e:
 *               K(t) = sum [max(x, 0) + log d] - t c0,   K'(t) = sum g_i (x >= 0 ? p_i / d : p_i e / d) - c0,   K''(t) = sum g_i^2 al be e / d^2.
 *           For each side sigma = +1, -1, with q = sigma |U| and b = (sigma > 0 ? G+ : G-) - c0: the side is outside the support iff
 *           sigma (b - q) <= 2^-30 A.  Otherwise Newton from t = 0 with the bracket (lo, hi) = (-inf, +inf): evaluate f = K'(t) - q; f < 0: lo = t, else
 *           hi = t; t' = t - f / K''(t); t' not finite: the side fails; |t' - t| <= tol |t'|: t^ = t' is accepted; else a t' not strictly inside (lo, hi)
 *           is replaced by (lo + hi) / 2 (not finite: the side fails), and t = t'.  At most max_iter such evaluations, else the side fails (the one
 *           evaluation of K and K'' at the accepted t^ is not counted).  At t^: w = sign(t^) sqrt(2 (t^ q - K(t^))), v = t^ sqrt(K''(t^)),
 *           zeta = w + log(v / w) / w (not finite: the side fails), tail = erfc(sigma zeta sqrt(1/2)) / 2.
 *           The observed side is sigma = +1 if U >= 0, else -1.
 *   flag 2  the observed side is outside the support or fails, or the opposite side fails: pval = erfc(|z| sqrt(1/2)), the normal p-value.
 *   flag 1  otherwise: pval = the observed side's tail + the opposite side's tail (0 where the opposite side is outside the support).
 * Every sum over the individuals runs in an order fixed by indiv alone, no atomics; the list of items is compacted by prefix sums.  Results are identical from
 * run to run, between host and device pointers, for every row-chunk size of the staging (MXA_ASSOC_CHUNK_ROWS) and every batch size of the correction
 * (MXA_ASSOC_SPA_BATCH = marked SNPs per batch, MXA_ASSOC_SPA_ITEMS = items per batch, never below the n items of one SNP; default: what fits 4 GiB of g,
 * and for a host matrix a bounce buffer of 256 MiB).  They carry the device's
 * exp / log / erfc and its contraction of a * b + c, so they are NOT promised bit-equal to any host evaluation, and as before NOT bit-identical between
 * column counts n (kh + 2).  One host wait (the number of items, with their list) lies between the scan and the correction.
 * pval (required): snps x n doubles, ld ldo; flag (optional): snps x n ints, ld ldo.  score, var, zstat and pval are all host or all device pointers, flag is
 *   on pval's side; plink, P, R, Wt and H are host or device pointers, each independently; nothing is written beyond row snps - 1 of a column.  Errors (return
 *   1, mxa_last_error() == 1, outputs untouched, all decided before a device is selected): every error of mxa_assoc_score; NULL P or pval; ldp < indiv;
 *   z_cutoff negative or NaN (+inf is legal: nothing is corrected); tol not in (0, 1); max_iter < 1; mixed host and device pointers among score, var, zstat,
 *   pval and flag.  12: not enough device memory (what mxa_assoc_score lists; P, tau, the lists, and one batch of g at its largest). */
int mxa_assoc_score_spa(const unsigned char *plink, int snps, int indiv, const double *P, long ldp, const double *R, long ldr, const double *Wt, long ldw,
                        const double *H, long ldh, int n, int kh, double z_cutoff, double tol, int max_iter, double *score, double *var, double *zstat,
                        double *pval, long ldo, int *flag, int *nobs);

/* The score test with effect sizes: mxa_assoc_score unchanged, then every (SNP s, trait c) with |z| >= z_cutoff gets the log odds ratio of the SNP, its
 * standard error and the likelihood-ratio statistic from a one-parameter logistic fit on the device, by maximum likelihood (penalty == 0) or with Firth's
 * penalty (penalty == 1).  The one-step estimate U / V is badly biased for rare alleles and rare cases, and the maximum-likelihood estimate does not exist where
 * carriers and cases separate; the penalised estimate always exists.  Like the saddlepoint p-value the fit sums transcendental functions of the
 * covariate-adjusted genotype over all individuals, once per Newton step, which no wrapper can form without the rows.
 * plink, P, R, Wt, H, n, kh, score, var, zstat and nobs are those of mxa_assoc_score_spa, and score, var, zstat and nobs receive bit for bit what
 * mxa_assoc_score returns for the same operands.  The model: logit pi_i(beta) = logit p_i + beta g_i -- the null model's linear predictor is the offset, the
 * adjusted genotype g the regressor.  With K the centred cumulant generating function of mxa_assoc_score_spa its log likelihood ratio against beta = 0 is
 * beta U - K(beta), its score U - K'(beta), its information K''(beta): no y is needed.  Firth's penalty adds log(K''(beta)) / 2.
 * Per (s, c), with mu, U, V, z and a_j of mxa_assoc_score's chain and g, c0, A, G+, G-, e, al, be, d, K, K', K'' exactly as defined for mxa_assoc_score_spa
 * (t = beta: x = beta g_i, e = exp(-|x|)):
 *   flag 3  z is not finite: beta = se = chisq = pval = NaN.
 *   flag 0  |z| < z_cutoff: the one-step values beta = U / V, se = 1 / sqrt(V), chisq = z * z, pval = erfc(|z| sqrt(1/2)), each operation rounded once.
 *   else    a fit.  Further sums: with pi_i = (x >= 0 ? p_i / d : p_i e / d) and omega_i = al be e / d^2:
 *               K'''(beta) = sum g_i^3 omega_i (1 - 2 pi_i),   K''''(beta) = sum g_i^4 omega_i (1 - 6 omega_i).
 *           The function to solve: penalty == 0: f = K'(beta) - U, f' = K''(beta); penalty == 1: f = K'(beta) - U - (K''' / K'') / 2,
 *           f' = K'' - (K'''' / K'' - (K''' / K'')^2) / 2, and where this f' is not positive K'' stands in for it.
 *           penalty == 0 only: the statistic is outside the support iff sigma (b - U) <= 2^-30 A with sigma = +1 if U >= 0 else -1 and
 *           b = (sigma > 0 ? G+ : G-) - c0 (the observed side of mxa_assoc_score_spa): the likelihood has no maximum.  With the penalty there is no such
 *           test: the penalised root exists on the edge of the support too.
 *           Newton from beta = 0 with the bracket (lo, hi) = (-inf, +inf): evaluate f and f'; f < 0: lo = beta, else hi = beta; beta' = beta - f / f';
 *           beta' not finite: the fit fails; |beta' - beta| <= tol |beta'|: beta^ = beta' is accepted; else a beta' not strictly inside (lo, hi) is
 *           replaced by (lo + hi) / 2 (not finite: the fit fails), and beta = beta'.  At most max_iter such evaluations, else the fit fails.  The first
 *           evaluation is at beta = 0 and yields K''(0); one evaluation of K and K'' at the accepted beta^ is not counted.
 *   flag 2  the statistic is outside the support (penalty == 0), the fit fails, or se or chisq below is not finite: the one-step values of flag 0.
 *           A first step that saturates every exp (fitted probabilities of some 1e-5 and less at the carriers with kh = 0, so that exp(-|beta g_i|) = 0
 *           and K'' = 0 at the second evaluation; or p_i in {0, 1} at the carriers, K''(0) = 0 at the first) makes beta' not finite: a failed fit
 *           with the one-step values.
 *   flag 1  otherwise: beta = beta^, se = 1 / sqrt(K''(beta^)), chisq = max(0, 2 (beta^ U - K(beta^)) + penalty log(K''(beta^) / K''(0))),
 *           pval = erfc(sqrt(chisq / 2)).
 * Every sum over the individuals runs in an order fixed by indiv alone, no atomics; list, items, batches and g are those of mxa_assoc_score_spa, and
 * MXA_ASSOC_CHUNK_ROWS, MXA_ASSOC_SPA_BATCH and MXA_ASSOC_SPA_ITEMS apply as they do there (the default batch: what fits 8 GiB of g -- one workgroup an item --, beyond 1024 items cut down to a multiple of 1024).  Results are identical from run to run, between host and device
 * pointers, for every row-chunk size of the staging and every batch size.  They carry the device's exp / log / erfc and its contraction of a * b + c, so they
 * are NOT promised bit-equal to any host evaluation, and as before NOT bit-identical between column counts n (kh + 2).  One host wait (the number of items, with
 * their list) lies between the scan and the fits.  Saddlepoint p-values and the fit in one call are not offered: call both entries.
 * beta (required), se, chisq, pval (optional): snps x n doubles, ld ldo; flag (optional): snps x n ints, ld ldo.  score, var, zstat, beta, se, chisq and pval
 *   are all host or all device pointers, flag is on beta's side; plink, P, R, Wt and H are host or device pointers, each independently; nothing is written
 *   beyond row snps - 1 of a column.  Errors (return 1, mxa_last_error() == 1, outputs untouched, all decided before a device is selected): every error of
 *   mxa_assoc_score_spa with beta in pval's place; penalty not 0 or 1.  12: not enough device memory (what mxa_assoc_score_spa lists, and the further snps x n
 *   result arrays). */
int mxa_assoc_score_firth(const unsigned char *plink, int snps, int indiv, const double *P, long ldp, const double *R, long ldr, const double *Wt, long ldw,
                          const double *H, long ldh, int n, int kh, double z_cutoff, int penalty, double tol, int max_iter, double *score, double *var,
                          double *zstat, double *beta, double *se, double *chisq, double *pval, long ldo, int *flag, int *nobs);

/* Set-based association: burden and SKAT statistics of SNP sets (genes, masks of rare variants, regions) under the null models of mxa_assoc_score.
 * mxa_assoc_score runs unchanged; the set stage follows it on the device.  plink, R, Wt, H, n, kh, score, var, zstat, ldo and nobs are those of
 * mxa_assoc_score; score, var, zstat and nobs are ALL optional here, and any of them that is given receives bit for bit what mxa_assoc_score returns for the
 * same operands.  A linear model passes R = residual / sigma^2, Wt = 1 / sigma^2, H = W C L^-T.
 * The sets are a CSR list on the HOST: set_ptr has nsets + 1 entries, non-decreasing, set_ptr[0] == 0; set_idx has set_ptr[nsets] SNP indices in [0, snps), in
 * any order; sets may overlap and a SNP may repeat within a set (no special case); set_wt (nullable: all ones) is parallel to set_idx and holds the variant
 * weights omega.  The size m_k = set_ptr[k + 1] - set_ptr[k] of a set satisfies 0 <= m_k <= 1024 (Phi of one (set, trait): at most 8 MiB).
 * Per set k and trait c, for its entries j, j' with s = set_idx[j]; mu, U_j and a_jh the scan's own values of SNP s (mxa_assoc_score's chain), w_c,i the
 * trait's working weights and x_j,i the allele count of individual i with missing calls replaced by mu (padding fields are not individuals):
 *   S_jj'   = sum_i x_j,i (w_c,i x_j',i) for j <= j', on the fp64 matrix unit: the product w x rounded once, the sum over the individuals in pieces of 4096
 *             (each piece: four interleaved runs of 64-genotype words, added as (r0 + r1) + (r2 + r3)), the pieces added in ascending order;
 *   Phi_jj' = S_jj', then for h ascending Phi_jj' = fma(-a_jh, a_j'h, Phi_jj'); computed for j <= j' and mirrored: Phi_jj' == Phi_j'j bit for bit;
 *   A_jj'   = (omega_j Phi_jj') omega_j', each product rounded once;
 *   B = sum_j omega_j U_j,  Q = sum_j (omega_j U_j)^2,  c1 = sum_j A_jj  over ascending j;
 *   varB = sum_jj' A_jj',  c2 = sum_jj' A_jj'^2,  c4 = sum_jj' ((A A)_jj')^2 with (A A)_jj' = the chain fma(A_jl, A_lj', .) over ascending l, never stored:
 *             per tile of 16 rows j a fixed tree over the columns j', the tiles added in ascending order.
 * The burden test is B / sqrt(varB) (p = erfc(|B| / sqrt(2 varB)), a wrapper's line), the SKAT statistic is Q, and mxa_assoc_skat_pvalue turns (Q, c1, c2, c4)
 * into its p-value.  An empty set gives zeros.  A SNP without any called individual (N = 0) makes the results of the sets that contain it non-finite and touches
 * no other set.
 * stat (required): nsets x 6 n doubles, column-major, ld lds >= nsets: column 6 c + t holds for trait c B (t = 0), varB (1), Q (2), c1 (3), c2 (4), c4 (5);
 *   nothing is written beyond row nsets - 1.  phi (optional): n sum_k m_k^2 doubles, the block of (k, c) is m_k x m_k column-major at the offset
 *   n sum_{k' < k} m_k'^2 + c m_k^2 (for SKAT-O, Davies or Kuonen p-values from eigenvalues, which this library does not offer).
 *   score, var, zstat, stat and phi are all host or all device pointers; plink, R, Wt and H are host or device pointers, each independently.
 * Every sum over the individuals runs in an order fixed by indiv alone, every sum over a set in an order fixed by m_k alone, no atomics: results are identical
 * from run to run, between host and device pointers, for every MXA_ASSOC_CHUNK_ROWS and for every batch size of the set stage, and a set's results do not
 * depend on which other sets are in the call.  As before they are NOT bit-identical between column counts n (kh + 2).  The stage works in batches of consecutive
 * sets: a batch is cut where its S / Phi blocks and partial sums would exceed 1 GiB, or its set entries MXA_ASSOC_SET_BATCH (environment, read per call, for
 * tests; default: no limit on the entries); it never holds less than one whole set.  The rows of a batch's distinct SNPs of a host matrix are copied to a
 * bounce buffer (runs of neighbouring rows in one copy); a device matrix is read in place.
 * Errors (return 1, mxa_last_error() == 1, outputs untouched, all decided before a device is selected): every error of mxa_assoc_score except its "score, var
 *   and zstat are all NULL"; nsets < 1; NULL set_ptr, set_idx or stat; set_ptr[0] != 0 or set_ptr decreasing; an index outside [0, snps) (the message names
 *   the set and the entry); m_k > 1024; lds < nsets; mixed host and device pointers among the results.  12: not enough device memory (what mxa_assoc_score
 *   lists, a score array where none is given, and of the stage: the bounce rows of its largest batch, one batch of S / Phi with its partial sums of 2 KiB per
 *   (set, trait, tile pair, piece), the batch's lists, and the device copy of a host stat). */
int mxa_assoc_set(const unsigned char *plink, int snps, int indiv, const double *R, long ldr, const double *Wt, long ldw, const double *H, long ldh, int n, int kh,
                  int nsets, const long *set_ptr, const int *set_idx, const double *set_wt, double *score, double *var, double *zstat, long ldo, int *nobs,
                  double *stat, long lds, double *phi);
/* The SKAT p-value of `count` items, on the host (no device is needed): Q = sum lambda_i chi^2_1 with the eigenvalues lambda of a positive semi-definite A is
 * matched to a scaled central chi-square by c1 = tr A, c2 = tr A^2, c4 = tr A^4 (Liu's moment matching in its modified form; by Cauchy-Schwarz c3^2 <= c2 c4,
 * so its non-central branch is never taken): l = c2^2 / c4, x = (Q - c1) sqrt(l / c2) + l, pval = the regularised upper incomplete gamma function
 * Q(l / 2, x / 2), and exactly 1 where x <= 0.  Sums in long double on the log scale, the series for x / 2 < l / 2 + 1 and the continued fraction otherwise:
 * tails down to the smallest doubles keep a relative error below 2^-40.  A non-finite Q, c1, c2 or c4, or c2 <= 0 or c4 <= 0, gives NaN (also in df).
 * df (nullable) receives l.  Errors (return 1, error 1): count < 0; a NULL Q, c1, c2, c4 or pval with count > 0. */
int mxa_assoc_skat_pvalue(long count, const double *Q, const double *c1, const double *c2, const double *c4, double *pval, double *df);

/* multiply engine of dgemm_compressed (process-wide; MXA_ENGINE in the environment sets the initial one).  Details and error bounds: DESIGN.md 3.2 / 3.3.
 *
 *   id  MXA_ENGINE   arithmetic                                                                     host waits
 *   0   (default)    n >= 7: fp64 MFMA, the reference's FMA chains; n <= 6 and the 1-3 odd columns   never
 *                    of n = 4q + r: exact int8 slicing of B when a device-side check proves it
 *                    exact (|err| <= 3.02 (S-1) 2^-53 sum|z b|), else fp64
 *   1   i8           int8 slicing for every n, 7 digits per column, no exactness check               never
 *   3   f64-strict   fp64 for every n (n <= 2: pair tables)                                          never
 *   4   i8-exact     int8 slicing for every n with the digit count chosen per call so that B is      once per call
 *                    represented without error (S <= 24; otherwise engine 0's path)
 *
 * Only engine 0 is ever the benchmark's `value`.  Ids 2 and 5 (small-n-i8, i8-guarded; rounds 3-5) are retired.
 * mxa_set_engine returns the previous id; an invalid id leaves the engine unchanged.
 * mxa_last_path: kernel family of the MAIN part of the most recent product (the 4q columns of a peeled n = 4q + r; the peeled columns carry their own
 * device-side verdict, which is not reported): 0 = k_gemm, 1 = k_lut (fp64 pair tables), 2 = k_gemm_i8 / k_gemm_i8_tn, 3 = fp64 behind a declined
 * exactness check (read from the device when this is called). */
int mxa_set_engine(int engine);
int mxa_get_engine(void);
int mxa_last_path(void);
/* Range of the fp64 MFMA path.  k_gemm feeds the genotype operand as the denormal double z * 2^-1074 and scales every column of B by a
 * power of two so that its largest |entry| sits just below 2^900; products of entries up to 847 binades below their column's largest
 * one are then normal doubles and every result equals the plain fp64 FMA chain of the reference
 * (src/cuda/dgemm_compressed_cuda.h:259-266) bit for bit.  A per-call check on the device finds columns whose non-zero entries span more
 * than 800 binades (about 240 decades) or hold inf / NaN; the product is then redone with plain fp64 operands (v_cvt_f64_u32, no
 * scaling) -- same arithmetic as the reference for every input, at twice the time for such calls.  mxa_last_range_fallback: 1 if the
 * most recent fp64-MFMA product on this (single-device) object took that fallback, 0 if not, -1 if unknown. */
int mxa_last_range_fallback(void *compressed);

/* measurement: HIP-event timing of the dominant kernel on the stream it is launched on.
 * mxa_profile_reset() clears the counters; after some dgemm_compressed / snp_multiply_gpu calls
 * mxa_profile_get() returns the number of dominant-kernel launches and their summed duration in ms. */
void mxa_profile_reset(void);
void mxa_profile_get(int *launches, double *total_ms);

/* geometry of the last dgemm_compressed call (for roofline accounting): rows, inner dim, n, split count */
void mxa_last_geometry(long *m, long *k, int *n, int *splits, int *a_tile, int *c_tile);
/* doubles of split-K partial sums the fp64 MFMA launch of an m x k x n product writes (no device needed: tests check that the plan of the
 * columns left after a peel, which can be LARGER than the plan of all n columns, never outgrows the workspace) */
long mxa_plan_partial_doubles(long m, long k, int n);
/* One packed copy per object (round 5 default; a property of the object from plink2compressed / mxa_bed2compressed / mxa_plink2compressed_shard /
 * mxa_plink2compressed_begin on).  Only the SNP-major copy is stored -- half the HBM (config 5 at its full 2M x 100k: 50 GB instead of 100; config 4 at its
 * full 5M x 200k: 250 GB, on one device) and half the staging upload; plink_transposed is not read.  Both products read that one copy: 'T' in the plain
 * form of k_gemm (output rows = packed rows), 'N' in the transposed-operand form (output rows = packed columns); since round 5 the two forms share one
 * permuted K order and run at the same rate (0.957-0.962 of the fp64 MFMA peak at BASELINE config 2; bit-identical results).  The exact int8 route of
 * n <= 6 and of peeled columns: 'T' on k_gemm_i8, 'N' on k_gemm_i8_tn (n <= 3: one digit tile, a CG step within 2 % of a two-copy object's; n = 4..6: two
 * tiles in ONE pass over the matrix, 1.44-1.50 ms against 1.3 on 500k x 50k; the fp64 tile would take 3.2-4.4).
 * MXA_SINGLE_ORIENTATION=0 in the environment of the creating call asks for BOTH copies (what rounds 1-4 stored): 'N' then runs the plain kernels
 * everywhere (4 <= n <= 6: 10-15 % faster), and the opt-in engines i8 / i8-exact multiply 'N' at wide n on the plain int8 kernel (on a one-copy object: on the transposed-operand kernel in column chunks of at most six digit tiles, one pass over the packed matrix per two tiles).  If the two copies do not fit the
 * device's free memory and one does, one is kept and a line on stderr says so (the reference reports "Not enough device memory" there,
 * cuda_utils.cu:162-185); a multi-device object decides once for all its shards.  Results of one-copy and two-copy objects agree to rounding
 * (bit-identical on the fp64 MFMA path and for integer-valued operands).  mxa_single_orientation: 1 / 0 (multi-device object: of its shards), -1 for an
 * invalid handle. */
int mxa_single_orientation(void *compressed);
/* capacity (doubles) of the partial-sum workspace an object holds right now; -1 for an invalid / multi-device object */
long mxa_partial_capacity(void *compressed);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* MIRACULIX_AMD_H */
