// mxa_stage.cpp -- staging of a device object: raw PLINK rows (host or device memory, or a .bed file) into the packed, tiled layout of PackedMatrix; creation,
// incremental filling, sealing and destruction of a Handle.  Mirrors plink2gpu of the reference (src/cuda/dgemm_compressed_cuda.cu:43-170).
#include "../../include/miraculix_amd.h"
#include "mxa_internal.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

namespace mxa {

// ------------------------------------------------------------------------------------------------ staging
thread_local int tl_single_override = -1;

// dimensions of a packed matrix of `rows` x `k` genotypes, nothing stored (d == nullptr): the padded layout stage_matrix and begin_handle allocate, and
// what a single-orientation object knows of the copy it does not keep
static void describe_matrix(PackedMatrix &M, long rows, long k) {
  M.d = nullptr; M.rows = rows; M.k = k;
  M.rows_pad = (rows + kRowAlign - 1) / kRowAlign * kRowAlign;
  M.k_pad = (k + kSlabK - 1) / kSlabK * kSlabK;
  M.pitch = (size_t)M.k_pad / 4;
  M.nslabs = M.k_pad / kSlabK;
}

// Raw PLINK rows in HOST memory (pitch src_pitch) into rows [row0, row0 + nrows) of M: row chunks of at most 256 MB go through a device bounce buffer
// (compacting the pitch) and are recoded on the device; d_freq (nullable): the allele frequencies of the rows are counted from the same chunks.  Every chunk
// is waited for: the bounce buffer is reused, and on return the caller may reuse its rows.
static int recode_host_rows(PackedMatrix &M, const uint8_t *src, size_t src_pitch, long row0, long nrows, long k, double *d_freq, hipStream_t s) {
  const long row_bytes = (k + 3) / 4;
  const long chunk_rows = stage_chunk_rows(nrows, (size_t)row_bytes, (size_t)256 << 20);   // (MXA_STAGE_CHUNK_ROWS: tests)
  uint8_t *bounce = nullptr;
  MXA_HIP(hipMalloc(reinterpret_cast<void **>(&bounce), (size_t)chunk_rows * row_bytes));
  int rc = 0;
  for (long r0 = 0; r0 < nrows && !rc; r0 += chunk_rows) {
    const long nr = std::min(chunk_rows, nrows - r0);
    hipError_t e;
    if ((size_t)row_bytes == src_pitch) e = hipMemcpyAsync(bounce, src + (size_t)r0 * src_pitch, (size_t)nr * row_bytes, hipMemcpyHostToDevice, s);
    else e = hipMemcpy2DAsync(bounce, row_bytes, src + (size_t)r0 * src_pitch, src_pitch, row_bytes, nr, hipMemcpyHostToDevice, s);
    if (!check_hip(e, __func__, __LINE__)) { rc = 1; break; }
    rc = launch_recode(bounce, row_bytes, row0 + r0, nr, k, 0, M, s);
    if (!rc && d_freq) rc = launch_allele_freq(bounce, nr, k, d_freq + r0, s);
    if (!rc && !check_hip(hipStreamSynchronize(s), __func__, __LINE__)) rc = 1;
  }
  (void)hipFree(bounce);
  return rc;
}

// Allocate the padded device layout for `rows` x `k` genotypes and fill it from raw PLINK rows (host or device).
static int stage_matrix(PackedMatrix &M, const uint8_t *src, size_t src_pitch, long rows, long k, hipStream_t s) {
  describe_matrix(M, rows, k);
  const size_t bytes = (size_t)M.rows_pad * M.pitch;
  MXA_HIP(hipMalloc(reinterpret_cast<void **>(&M.d), bytes));
  MXA_HIP(hipMemsetAsync(M.d, 0, bytes, s));
  int src_dev = -1;
  if (ptr_location(src, &src_dev) != 1) return recode_host_rows(M, src, src_pitch, 0, rows, k, nullptr, s);
  int cur = 0;
  MXA_HIP(hipGetDevice(&cur));
  if (src_dev != cur) {   // the recode kernel reads the other GPU's memory over xGMI
    if (!enable_peer(cur, src_dev)) { set_error(15, "plink2compressed: device %d cannot read the source matrix in the memory of device %d (peer access not available or could not be enabled)", cur, src_dev); return 1; }
    if (sync_foreign_producer(src_dev)) return 1;   // the matrix may still be being written by work on the source device's default stream
  }
  if (launch_recode(src, src_pitch, 0, rows, k, 0, M, s)) return 1;
  MXA_HIP(hipStreamSynchronize(s));
  return 0;
}

// Both orientations from the SNP-major PLINK matrix alone: the raw bytes are brought to the device once (a host source: one compact upload;
// a device source is used in place), recoded into the SNP-major object, transposed on the device (raw PLINK codes, so a missing 01 stays a
// missing 01) and the transposed bytes recoded into the individual-major object -- bit-identical to staging a caller-supplied transposed
// copy.  Temporary device memory: the raw matrix (host sources only) + its transpose, released before the workspace is allocated.
static int stage_from_snp_major(Handle *h, const uint8_t *plink, size_t plink_pitch) {
  const long snps = h->snps, indiv = h->indiv;
  const size_t bps = ((size_t)indiv + 3) / 4, bpi = ((size_t)snps + 3) / 4;
  hipStream_t s = h->stream;
  int src_dev = -1;
  const bool src_on_device = ptr_location(plink, &src_dev) == 1;
  uint8_t *d_raw = nullptr, *d_raw_t = nullptr;
  int rc = 0;
  const uint8_t *d_src = plink;
  size_t d_pitch = plink_pitch;
  if (!src_on_device || src_dev != h->device || plink_pitch != bps) {   // compact copy on this device (the transpose kernels want pitch = ceil(indiv/4))
    if (src_on_device && src_dev != h->device && sync_foreign_producer(src_dev)) return 1;
    MXA_HIP(hipMalloc(reinterpret_cast<void **>(&d_raw), (size_t)snps * bps));
    hipError_t e = plink_pitch == bps ? hipMemcpyAsync(d_raw, plink, (size_t)snps * bps, hipMemcpyDefault, s)
                                      : hipMemcpy2DAsync(d_raw, bps, plink, plink_pitch, bps, snps, hipMemcpyDefault, s);
    if (!check_hip(e, __func__, __LINE__) || !check_hip(hipStreamSynchronize(s), __func__, __LINE__)) { (void)hipFree(d_raw); return 1; }
    d_src = d_raw; d_pitch = bps;
  }
  rc = stage_matrix(h->snp_major, d_src, d_pitch, snps, indiv, s);
  if (!rc && !check_hip(hipMalloc(reinterpret_cast<void **>(&d_raw_t), (size_t)indiv * bpi), __func__, __LINE__)) rc = 1;
  if (!rc) rc = launch_transpose_2bit(d_src, snps, indiv, d_raw_t, s);
  if (!rc && !check_hip(hipStreamSynchronize(s), __func__, __LINE__)) rc = 1;
  if (d_raw) { (void)hipFree(d_raw); d_raw = nullptr; }
  if (!rc) rc = stage_matrix(h->ind_major, d_raw_t, bpi, indiv, snps, s);
  if (d_raw_t) (void)hipFree(d_raw_t);
  return rc;
}

void destroy_handle(Handle *h) {
  if (!h) return;
  {   // mxa_last_path() must not read a flag of this object once its memory is gone
    std::lock_guard<std::mutex> lk(g_prof_mutex);
    Geometry &geo = last_geometry();
    if (geo.d_flag && h->ws.d_denflag && geo.d_flag >= h->ws.d_denflag && geo.d_flag < h->ws.d_denflag + 4) { geo.d_flag = nullptr; if (geo.path == 4) geo.path = 2; }
  }
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  void *ptrs[] = {h->snp_major.d, h->ind_major.d, h->d_f, h->ws.d_Bstage, h->ws.d_Cstage, h->ws.d_Bp, h->ws.d_P, h->ws.d_colpart, h->ws.d_i8, h->ws.d_tmp, h->ws.d_exp, h->ws.d_denflag};
  for (void *p : ptrs) if (p) (void)hipFree(p);
  for (hipEvent_t e : {h->ev0[0], h->ev0[1], h->ev1[0], h->ev1[1], h->ev_in[0], h->ev_in[1], h->ev_out[0], h->ev_out[1]}) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->pev) if (e) (void)hipEventDestroy(e);
  for (hipStream_t ps : h->pipe) if (ps) (void)hipStreamDestroy(ps);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  free(h->h_f);
  h->magic = 0;
  delete h;
}

int single_orientation_policy() {
  // Round 5: ONE packed copy (SNP-major) is the default -- both products read it at the rate two copies reach (fp64 MFMA: plain form = transposed form =
  // 0.957-0.962 of the peak; the CG step within 2 %), for half the HBM and half the staging.  MXA_SINGLE_ORIENTATION=0 asks for both copies (the opt-in: 'N'
  // with 4 <= n <= 6 columns then runs the plain int8 kernel in one pass instead of two); they are kept when they fit the device's free memory, otherwise
  // one copy is kept and a line on stderr says so (the reference reports "Not enough device memory" there, cuda_utils.cu:162-185).
  const char *e = getenv("MXA_SINGLE_ORIENTATION");
  if (!e || !*e) return 1;
  return atoi(e) != 0 ? 1 : 2;
}

size_t object_footprint(long snps, long indiv, int max_n, bool single) {
  return (size_t)((snps + kRowAlign) * ((indiv + kSlabK) / 4)) + (single ? 0 : (size_t)((indiv + kRowAlign) * ((snps + kSlabK) / 4))) +
         (size_t)3 * sizeof(double) * (size_t)std::max(snps, indiv) * (size_t)std::max(max_n, 1);
}

// What create_handle and begin_handle share ahead of the staging: the options default, the refusal of use_gpu=0, the device (device < 0: select_device), the
// memory pre-flight like checkDevMemory (cuda_utils.cu:162-185), the Handle and its stream.  need_bytes(free bytes) -> device bytes of the object (create_handle
// decides there whether it keeps one packed copy or two).  `who` starts the messages.  nullptr: an error was reported.
template <typename Need>
static Handle *new_handle(const char *who, long snps, long indiv, int max_n, int device, bool banner, Need &&need_bytes) {
  Options &o = options();
  if (!o.set) {  // reference default before any user call: gpu when compiled with CUDA, centred (5codesChar.cc:127-143)
    o.gpu = true; o.centered = true; o.set = true;
  }
  if (!o.gpu) { set_error(14, "%s: setOptions_compressed was called with use_gpu=0; this library has no CPU engine", who); return nullptr; }
  int dev = device;
  if (dev < 0) dev = select_device();
  else if (!check_hip(hipSetDevice(dev), __func__, __LINE__)) dev = -1;
  if (dev < 0) return nullptr;
  if (banner && (env_print_level() > 0 || o.print_level > 0)) {
    hipDeviceProp_t prop;
    print_compile_info("dgemm_compressed");
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) printf("miraculix_amd - dgemm_compressed: using device %s [%s] (device no %d).\n", prop.name, prop.gcnArchName, dev);
  }
  size_t free_b = 0, total_b = 0;
  if (!check_hip(hipMemGetInfo(&free_b, &total_b), __func__, __LINE__)) return nullptr;
  const size_t need = need_bytes(free_b);
  if (need > free_b) {
    set_error(12, "Not enough device memory available. Required %zu GB, free %zu GB, total on device %zu GB", need >> 30, free_b >> 30, total_b >> 30);
    return nullptr;
  }
  Handle *h = new Handle();
  h->device = dev; h->snps = snps; h->indiv = indiv; h->max_n = std::max(max_n, 1);
  // a BLOCKING stream: it orders itself against the legacy default stream, so device-resident B produced by work the caller
  // enqueued on the default stream (e.g. PyTorch ops) is complete before k_pack_B reads it, and later default-stream work sees
  // C.  Callers on other streams pass theirs to mxa_dgemm_compressed_device.
  if (!check_hip(hipStreamCreateWithFlags(&h->stream, hipStreamDefault), __func__, __LINE__)) { destroy_handle(h); return nullptr; }
  return h;
}

// the allele frequencies of an object: snps doubles on the device and their host copy (zeros until filled)
static int alloc_freq(Handle *h, const char *who) {
  MXA_HIP(hipMalloc(reinterpret_cast<void **>(&h->d_f), sizeof(double) * h->snps));
  h->h_f = (double *)calloc((size_t)h->snps, sizeof(double));
  if (!h->h_f) { set_error(12, "%s: out of host memory for %ld allele frequencies", who, h->snps); return 1; }
  return 0;
}

int create_handle(const uint8_t *plink, size_t plink_pitch, const uint8_t *plink_t, size_t plink_t_pitch, long snps, long indiv, const double *f,
                  int max_n, void **out, int device) {
  if (out) *out = nullptr;
  if (!out) { set_error(1, "plink2compressed: compressed is NULL"); return 1; }
  if (!plink) { set_error(1, "plink2compressed: plink is NULL"); return 1; }
  // plink_transposed NULL or the same pointer as plink: the reference's CPU path never reads it and its Fortran benchmark passes the same
  // pointer twice (5codesChar.cc:368-393, utils/benchmark/benchmark.f90:185).  Only the SNP-major matrix crosses PCIe then; the
  // individual-major copy is produced on the device (k_transpose_2bit*), as mxa_bed2compressed does.
  const bool one_pointer = !plink_t || plink_t == plink;
  if (snps <= 0 || indiv <= 0) { set_error(1, "plink2compressed: snps and indiv must be positive"); return 1; }
  // Where the reference gives up -- two packed copies do not fit -- this build keeps the SNP-major copy alone if THAT fits (MXA_SINGLE_ORIENTATION unset /
  // auto; Handle::single): both products then read the one copy.
  int src_dev0 = -1;
  bool single0 = false;
  Handle *h = new_handle("plink2compressed", snps, indiv, max_n, device, true, [&](size_t free_b) {
    const int policy = tl_single_override >= 0 ? tl_single_override : single_orientation_policy();
    const size_t need_two = object_footprint(snps, indiv, max_n, false), need_one = object_footprint(snps, indiv, max_n, true);
    // what the staging itself holds on top at its peak: a host source goes through a 256 MB bounce buffer; the one-pointer shape keeps the raw transposed
    // block (about one packed copy) until the second copy is built
    const size_t bounce = ptr_location(plink, &src_dev0) == 1 ? 0 : (size_t)256 << 20;
    const size_t tmp_two = one_pointer ? (size_t)indiv * (((size_t)snps + 3) / 4) + bounce : bounce, tmp_one = bounce;
    single0 = policy == 1 || (policy == 2 && need_two + tmp_two > free_b && need_one + tmp_one <= free_b);
    if (single0 && policy == 2)   // always said: the caller asked for two copies (mxa_single_orientation() reports what the object holds)
      fprintf(stderr, "miraculix_amd - dgemm_compressed: two packed copies need %.1f GB, %.1f GB are free: keeping the SNP-major copy only (%.1f GB).\n", need_two / 1e9, free_b / 1e9, need_one / 1e9);
    return single0 ? need_one : need_two;
  });
  if (!h) return 1;
  // decided above, a property of the object from then on: only the SNP-major copy is staged; plink_transposed is not read
  h->single = single0;
  if (h->single) {
    if (stage_matrix(h->snp_major, plink, plink_pitch, snps, indiv, h->stream)) { destroy_handle(h); return 1; }
    describe_matrix(h->ind_major, indiv, snps);
  } else
  if (one_pointer ? stage_from_snp_major(h, plink, plink_pitch) :
                    (stage_matrix(h->snp_major, plink, plink_pitch, snps, indiv, h->stream) ||
                     stage_matrix(h->ind_major, plink_t, plink_t_pitch, indiv, snps, h->stream))) { destroy_handle(h); return 1; }
  if (alloc_freq(h, "plink2compressed")) { destroy_handle(h); return 1; }
  if (f) {
    hipError_t e = hipMemcpy(h->d_f, f, sizeof(double) * snps, hipMemcpyDefault);
    if (!check_hip(e, __func__, __LINE__)) { destroy_handle(h); return 1; }
    h->has_f = true;
  } else {
    (void)hipMemset(h->d_f, 0, sizeof(double) * snps);
  }
  // (the host copy of the frequencies travels on the object's stream; that alone does NOT pay the runtime's first staged device-to-host copy of a product --
  // measured, "attempt 1" in profiles/r06_harness_phase_clock.txt -- the warm-up products below do)
  if (!check_hip(hipMemcpyAsync(h->h_f, h->d_f, sizeof(double) * snps, hipMemcpyDeviceToHost, h->stream), __func__, __LINE__) ||
      !check_hip(hipStreamSynchronize(h->stream), __func__, __LINE__)) { destroy_handle(h); return 1; }
  if (ensure_workspace(h, h->max_n) || reserve_small_routes(h, h->max_n)) { destroy_handle(h); return 1; }
  if (warm_up(h, src_dev0 < 0)) { destroy_handle(h); return 1; }
  *out = h;
  return 0;
}

// ---- incremental staging (round 5).  plink2compressed wants the whole PLINK matrix behind one pointer; at BASELINE config 4's full extent that is 250 GB
// next to the 250 GB object it becomes.  Here the object is allocated first (ONE packed copy, SNP-major: Handle::single) and filled by blocks of SNP rows
// -- from a generator, a file reader, another device -- so that nothing but the object and one block is ever resident.  The .bed reader uses it for
// single-orientation objects (bed_range_to_handle).
int begin_handle(long snps, long indiv, int max_n, void **out, int device) {
  if (out) *out = nullptr;
  if (!out) { set_error(1, "mxa_plink2compressed_begin: compressed is NULL"); return 1; }
  if (snps <= 0 || indiv <= 0) { set_error(1, "mxa_plink2compressed_begin: snps and indiv must be positive"); return 1; }
  // the packed copy + B in fragment order + at least one K split of partial sums (partial_budget cuts the rest into groups) + the staged operands' room
  Handle *h = new_handle("mxa_plink2compressed_begin", snps, indiv, max_n, device, false, [&](size_t) { return object_footprint(snps, indiv, max_n, true); });
  if (!h) return 1;
  h->single = true; h->staging = true;
  PackedMatrix &M = h->snp_major;
  describe_matrix(M, snps, indiv);
  const size_t bytes = (size_t)M.rows_pad * M.pitch;
  if (!check_hip(hipMalloc(reinterpret_cast<void **>(&M.d), bytes), __func__, __LINE__) ||
      !check_hip(hipMemsetAsync(M.d, 0, bytes, h->stream), __func__, __LINE__)) { destroy_handle(h); return 1; }
  describe_matrix(h->ind_major, indiv, snps);
  if (alloc_freq(h, "mxa_plink2compressed_begin") ||
      !check_hip(hipMemsetAsync(h->d_f, 0, sizeof(double) * snps, h->stream), __func__, __LINE__)) { destroy_handle(h); return 1; }
  h->has_f = true;
  if (ensure_workspace(h, h->max_n)) { destroy_handle(h); return 1; }
  *out = h;
  return 0;
}

int append_rows(Handle *h, const uint8_t *rows, long snp_begin, long nrows, const double *f_rows) {
  if (!h->staging) { set_error(19, "mxa_plink2compressed_rows: the object is sealed (or was not made by mxa_plink2compressed_begin)"); return 1; }
  if (!rows || snp_begin < 0 || nrows <= 0 || snp_begin + nrows > h->snps) {
    set_error(1, "mxa_plink2compressed_rows: need rows != NULL and 0 <= snp_begin, snp_begin + nrows <= snps (got [%ld, %ld) of %ld)", snp_begin, snp_begin + nrows, h->snps);
    return 1;
  }
  // coverage is an interval set, not a count: a block appended twice (a retried block) or overlapping another one is refused, so that an object can only
  // be sealed with every SNP row written exactly once
  auto at = std::lower_bound(h->staged_iv.begin(), h->staged_iv.end(), std::make_pair(snp_begin, snp_begin));
  if ((at != h->staged_iv.end() && at->first < snp_begin + nrows) || (at != h->staged_iv.begin() && std::prev(at)->second > snp_begin)) {
    set_error(1, "mxa_plink2compressed_rows: rows [%ld, %ld) overlap rows that were already appended", snp_begin, snp_begin + nrows);
    return 1;
  }
  MXA_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const long bps = (h->indiv + 3) / 4;
  int src_dev = -1;
  const bool on_dev = ptr_location(rows, &src_dev) == 1;
  if (f_rows) MXA_HIP(hipMemcpyAsync(h->d_f + snp_begin, f_rows, sizeof(double) * nrows, hipMemcpyDefault, s));
  double *d_count = (!f_rows && h->has_f) ? h->d_f + snp_begin : nullptr;   // frequencies counted on the device (has_f cleared: an object without frequencies, see mxa_internal.h)
  if (on_dev) {
    if (src_dev != h->device) {
      if (!enable_peer(h->device, src_dev)) { set_error(15, "mxa_plink2compressed_rows: device %d cannot read the rows in the memory of device %d", h->device, src_dev); return 1; }
      if (sync_foreign_producer(src_dev)) return 1;
    }
    if (launch_recode(rows, (size_t)bps, snp_begin, nrows, h->indiv, 0, h->snp_major, s)) return 1;
    if (d_count && launch_allele_freq(rows, nrows, h->indiv, d_count, s)) return 1;
    MXA_HIP(hipStreamSynchronize(s));   // the caller may reuse its block buffer
  } else if (recode_host_rows(h->snp_major, rows, (size_t)bps, snp_begin, nrows, h->indiv, d_count, s)) return 1;   // (compact rows only: pitch = ceil(indiv / 4))
  h->staged_rows += nrows;
  h->staged_iv.insert(at, {snp_begin, snp_begin + nrows});
  return 0;
}

int end_handle(Handle *h) {
  if (!h->staging) { set_error(19, "mxa_plink2compressed_end: the object is already sealed"); return 1; }
  long covered = 0, next = 0;          // the intervals are disjoint and sorted: full coverage = they chain from 0 to snps
  for (const auto &iv : h->staged_iv) { if (iv.first != next) break; next = iv.second; covered = next; }
  if (covered != h->snps) {
    set_error(1, "mxa_plink2compressed_end: %ld SNP rows were appended, the object has %ld (first row not yet appended: %ld)", h->staged_rows, h->snps, covered);
    return 1;
  }
  h->staged_iv.clear(); h->staged_iv.shrink_to_fit();
  MXA_HIP(hipSetDevice(h->device));
  MXA_HIP(hipMemcpyAsync(h->h_f, h->d_f, sizeof(double) * h->snps, hipMemcpyDeviceToHost, h->stream));   // (on the object's stream: see create_handle)
  MXA_HIP(hipStreamSynchronize(h->stream));
  h->staging = false;
  if (reserve_small_routes(h, h->max_n)) return 1;
  return warm_up(h, false);
}

// SNP rows [snp_begin, snp_end) of the SNP-major file `base`.bed -> object on `device`.  Only those rows are read (the reference
// reader streams the whole file row by row, read_plink.jl:161-222); the individual-major block and the allele frequencies of the
// range are produced on the device (k_transpose_2bit*, k_allele_freq), so no process ever needs the full individual-major matrix.
// File chunks go through two pinned buffers so that reading chunk c+1 overlaps the upload of chunk c.
int bed_range_to_handle(const char *base_c, long snps_total, long indiv, long snp_begin, long snp_end, int max_n, int device, void **out,
                        double *f_out_local) {
  if (out) *out = nullptr;
  const std::string base(base_c);
  if (!out || snps_total <= 0 || indiv <= 0 || snp_begin < 0 || snp_end > snps_total || snp_begin >= snp_end) {
    set_error(1, "bed staging: need 0 <= snp_begin < snp_end <= snps (got [%ld, %ld) of %ld) and indiv > 0", snp_begin, snp_end, snps_total);
    return 1;
  }
  FILE *fh = fopen((base + ".bed").c_str(), "rb");
  if (!fh) { set_error(1, "mxa_bed2compressed: cannot open %s.bed", base.c_str()); return 1; }
  unsigned char magic[3];
  if (fread(magic, 1, 3, fh) != 3 || magic[0] != 0x6c || magic[1] != 0x1b || magic[2] != 0x01) {
    fclose(fh);
    set_error(1, "mxa_bed2compressed: %s.bed is not a SNP-major PLINK .bed file (magic bytes 6c 1b 01 expected)", base.c_str());
    return 1;
  }
  const size_t bps = ((size_t)indiv + 3) / 4;
  const long rows = snp_end - snp_begin;
  const size_t bpi = ((size_t)rows + 3) / 4;
  // the reference reader fails on a file that is too short and asserts eof afterwards ("Too large .bed file", read_plink.jl:190-193)
  if (fseeko(fh, 0, SEEK_END) == 0) {
    const off_t sz = ftello(fh);
    if (sz >= 0 && (size_t)sz != 3 + (size_t)snps_total * bps) {
      fclose(fh);
      set_error(1, "mxa_bed2compressed: %s.bed has %lld bytes, expected 3 + %ld x ceil(%ld/4) = %zu", base.c_str(), (long long)sz, snps_total, indiv, 3 + (size_t)snps_total * bps);
      return 1;
    }
  }
  if (fseeko(fh, (off_t)(3 + (size_t)snp_begin * bps), SEEK_SET) != 0) { fclose(fh); set_error(1, "mxa_bed2compressed: cannot seek in %s.bed", base.c_str()); return 1; }
  int dev = device;
  if (dev < 0) dev = select_device();
  else if (!check_hip(hipSetDevice(dev), __func__, __LINE__)) dev = -1;
  if (dev < 0) { fclose(fh); return 1; }
  uint8_t *d_plink = nullptr, *d_plink_t = nullptr;
  double *d_f = nullptr;
  void *pin[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  hipStream_t cs = nullptr;
  int rc = 0;
  auto bad = [&](hipError_t e, int line) { if (e != hipSuccess) { check_hip(e, "mxa_bed2compressed", line); rc = 1; } return rc; };
  const size_t rows_per_chunk = (size_t)stage_chunk_rows(rows, bps, (size_t)64 << 20);   // (MXA_STAGE_CHUNK_ROWS: tests)
  const size_t chunk_bytes = rows_per_chunk * bps;
  // only the SNP-major copy will be kept (no transposed block is built): asked for, or the raw block + its transpose + the two packed copies do not fit
  bool single;
  {
    const int policy = tl_single_override >= 0 ? tl_single_override : single_orientation_policy();
    size_t free_b = 0, total_b = 0;
    if (bad(hipMemGetInfo(&free_b, &total_b), __LINE__)) goto out;
    const size_t raw = (size_t)rows * bps, raw_t = (size_t)indiv * bpi;
    single = policy == 1 || (policy == 2 && raw + raw_t + object_footprint(rows, indiv, max_n, false) > free_b && 2 * chunk_bytes + object_footprint(rows, indiv, max_n, true) <= free_b);
  }
  if (single) {
    // ONE packed copy: the file is streamed straight into the object (round 5) -- chunk c + 1 is read from the file while chunk c is uploaded, recoded into
    // the tiled layout and counted (k_recode, k_allele_freq), all on the object's stream; device memory beyond the object: two 64 MB chunks.  (Round 4 held
    // the raw matrix on the device beside the object: a 250 GB .bed could not become a 250 GB object.)
    uint8_t *dchunk[2] = {nullptr, nullptr};
    Handle *h = nullptr;
    {
      void *obj = nullptr;
      if (begin_handle(rows, indiv, max_n, &obj, dev)) { rc = 1; goto out; }
      h = reinterpret_cast<Handle *>(obj);
      *out = obj;
    }
    for (int i = 0; i < 2 && !rc; i++)
      if (bad(hipMalloc((void **)&dchunk[i], chunk_bytes), __LINE__) || bad(hipHostMalloc(&pin[i], chunk_bytes, hipHostMallocDefault), __LINE__) ||
          bad(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming), __LINE__)) break;
    {
      int slot = 0;
      bool used[2] = {false, false};
      for (size_t r0 = 0; r0 < (size_t)rows && !rc; r0 += rows_per_chunk, slot ^= 1) {
        const size_t nr = std::min(rows_per_chunk, (size_t)rows - r0);
        if (used[slot] && bad(hipEventSynchronize(ev[slot]), __LINE__)) break;     // upload and kernels that last used this pair of buffers are done
        if (fread(pin[slot], 1, nr * bps, fh) != nr * bps) { set_error(1, "mxa_bed2compressed: %s.bed is shorter than %ld x ceil(%ld/4) bytes", base.c_str(), snps_total, indiv); rc = 1; break; }
        if (bad(hipMemcpyAsync(dchunk[slot], pin[slot], nr * bps, hipMemcpyHostToDevice, h->stream), __LINE__)) break;
        if (launch_recode(dchunk[slot], bps, (long)r0, (long)nr, indiv, 0, h->snp_major, h->stream) ||
            launch_allele_freq(dchunk[slot], (long)nr, indiv, h->d_f + r0, h->stream)) { rc = 1; break; }
        if (bad(hipEventRecord(ev[slot], h->stream), __LINE__)) break;
        used[slot] = true;
      }
      if (!rc) bad(hipStreamSynchronize(h->stream), __LINE__);
    }
    if (!rc) { h->staged_rows = rows; h->staged_iv.assign(1, {0L, (long)rows}); rc = end_handle(h); }   // (the loop above wrote every row of the range exactly once)
    if (!rc && f_out_local) memcpy(f_out_local, h->h_f, sizeof(double) * rows);
    for (int i = 0; i < 2; i++) if (dchunk[i]) (void)hipFree(dchunk[i]);
    goto out;
  }
  if (bad(hipMalloc((void **)&d_plink, (size_t)rows * bps), __LINE__) || (!single && bad(hipMalloc((void **)&d_plink_t, (size_t)indiv * bpi), __LINE__)) ||
      bad(hipMalloc((void **)&d_f, sizeof(double) * rows), __LINE__) || bad(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking), __LINE__)) goto out;
  for (int i = 0; i < 2; i++)
    if (bad(hipHostMalloc(&pin[i], chunk_bytes, hipHostMallocDefault), __LINE__) || bad(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming), __LINE__)) goto out;
  {
    int slot = 0;
    bool used[2] = {false, false};
    for (size_t r0 = 0; r0 < (size_t)rows && !rc; r0 += rows_per_chunk, slot ^= 1) {
      const size_t nr = std::min(rows_per_chunk, (size_t)rows - r0);
      if (used[slot] && bad(hipEventSynchronize(ev[slot]), __LINE__)) break;     // the upload that last used this buffer is done
      if (fread(pin[slot], 1, nr * bps, fh) != nr * bps) { set_error(1, "mxa_bed2compressed: %s.bed is shorter than %ld x ceil(%ld/4) bytes", base.c_str(), snps_total, indiv); rc = 1; break; }
      if (bad(hipMemcpyAsync(d_plink + r0 * bps, pin[slot], nr * bps, hipMemcpyHostToDevice, cs), __LINE__) || bad(hipEventRecord(ev[slot], cs), __LINE__)) break;
      used[slot] = true;
    }
    if (!rc) bad(hipStreamSynchronize(cs), __LINE__);
  }
  if (!rc && !single) rc = launch_transpose_2bit(d_plink, rows, indiv, d_plink_t, nullptr);
  if (!rc) rc = launch_allele_freq(d_plink, rows, indiv, d_f, nullptr);
  if (!rc) bad(hipDeviceSynchronize(), __LINE__);
  if (!rc) {
    const int keep = tl_single_override;
    tl_single_override = single ? 1 : 0;     // the object follows the decision taken for the staging buffers
    rc = create_handle(d_plink, bps, d_plink_t, bpi, rows, indiv, d_f, max_n, out, dev);
    tl_single_override = keep;
  }
  if (!rc && f_out_local) bad(hipMemcpy(f_out_local, d_f, sizeof(double) * rows, hipMemcpyDeviceToHost), __LINE__);
out:
  fclose(fh);
  for (int i = 0; i < 2; i++) { if (pin[i]) (void)hipHostFree(pin[i]); if (ev[i]) (void)hipEventDestroy(ev[i]); }
  if (cs) (void)hipStreamDestroy(cs);
  if (d_plink) (void)hipFree(d_plink);
  if (d_plink_t) (void)hipFree(d_plink_t);
  if (d_f) (void)hipFree(d_f);
  if (rc && out && *out) { destroy_handle(reinterpret_cast<Handle *>(*out)); *out = nullptr; }
  return rc;
}
}  // namespace mxa
