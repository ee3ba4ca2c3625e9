// mxa_api.cpp -- host side of the C ABI (include/miraculix_amd.h): options singleton, error and profile state, the extern "C" entries.  Objects are
// staged in mxa_stage.cpp, products driven in mxa_product.cpp.  Mirrors the reference's L3/L2 layers (src/miraculix/5codesAPI.c,
// src/miraculix/5codesChar.cc:165-449) and the host part of src/cuda/dgemm_compressed_cuda.cu, re-designed so that
// nothing is allocated, created or destroyed per multiply and operands may already live in HBM.
//
// No CPU fallback: every compute entry needs a HIP device and fails loudly without one.
#include "../../include/miraculix_amd.h"
#include "mxa_internal.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace mxa {

// ------------------------------------------------------------------------------------------------ state
static int g_err = 0;
static char g_errmsg[512] = "";

Options &options() { static Options o; return o; }
Profile &profile() { static Profile p; return p; }
Geometry &last_geometry() { static Geometry g; return g; }
bool g_profile_on = true;
// multiply engine (include/miraculix_amd.h, mxa_set_engine): 0 = fp64 MFMA (default), 1 = int8 slicing, 3 = fp64 only, 4 = exact int8 slicing; ids 2 and 5 (rounds 3-5) are retired
std::atomic<int> g_engine{[] {
  const char *e = getenv("MXA_ENGINE");
  if (e && std::string(e) == "i8") return 1;
  if (e && std::string(e) == "f64-strict") return 3;
  if (e && std::string(e) == "i8-exact") return 4;
  return 0;
}()};

int env_print_level() {  // reference: cuda_utils.cu:44-52, env PRINT_LEVEL
  const char *e = getenv("PRINT_LEVEL");
  return e ? atoi(e) : 0;
}

// Banner of the reference (cuda_utils.cu:64-81: name, compile date, git commit), once per process; printed under PRINT_LEVEL > 0 /
// print_details only -- the reference prints it by default, this library is quiet unless asked.
#ifndef MXA_COMMIT_ID
#define MXA_COMMIT_ID "unknown"
#endif
void print_compile_info(const char *what) {
  static std::atomic<bool> done{false};
  if (done.exchange(true)) return;
  printf("------------------------------------------------------------\n\tmiraculix_amd (MI355X / gfx950) - %s\nCompiled on %s %s, git commit %s\n"
         "------------------------------------------------------------\n", what, __DATE__, __TIME__, MXA_COMMIT_ID);
}

// The status is per process, like the reference's (its entries return void and print).  Worker threads of a multi-device object
// report through the same state: the mutex keeps the message intact, the first error of a call wins.
std::mutex g_prof_mutex;   // profile() / last_geometry() are written by the worker threads of multi-device objects too
static std::mutex g_err_mutex;
void clear_error() { std::lock_guard<std::mutex> lk(g_err_mutex); g_err = 0; g_errmsg[0] = 0; }

void set_error(int code, const char *fmt, ...) {
  char msg[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, sizeof(msg), fmt, ap);
  va_end(ap);
  fprintf(stderr, "miraculix_amd: %s\n", msg);
  std::lock_guard<std::mutex> lk(g_err_mutex);
  if (g_err == 0) { g_err = code; memcpy(g_errmsg, msg, sizeof(g_errmsg)); }
}

bool check_hip(hipError_t e, const char *func, int line) {
  if (e == hipSuccess) return true;
  // wording follows the reference's checkError (cuda_utils.cu:83-90)
  set_error(100 + (int)e, "Internal error in function %s at line %d: %s", func, line, hipGetErrorString(e));
  return false;
}

void debug_info(const char *fmt, ...) {
  if (env_print_level() <= 0 && options().print_level <= 0) return;
  va_list ap;
  va_start(ap, fmt);
  printf("\t ");
  vprintf(fmt, ap);
  printf("\n");
  va_end(ap);
  fflush(stdout);   // (a caller that reads the line from a pipe or a file sees it when the call returns)
}

thread_local CallClock *tl_call_clock = nullptr;
double CallClock::now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
void CallClock::mark(const char *what) {
  if (!on) return;
  const double t = now();
  if (len < (int)sizeof(line) - 48) len += snprintf(line + len, sizeof(line) - len, " %s %.3f", what, (t - last) * 1e3);
  last = t;
}
void CallClock::report(const char *head) {
  if (!on) return;
  printf("\t %s: total %.3f ms |%s (ms)\n", head, (now() - t0) * 1e3, line);
  on = false;
}

static Handle *as_handle(void *p, const char *who) {
  Handle *h = reinterpret_cast<Handle *>(p);
  if (!h || h->magic != kMagic) {
    set_error(2, "%s: invalid or uninitialised compressed object", who);
    return nullptr;
  }
  return h;
}

int ptr_location(const void *p, int *dev) {
  if (dev) *dev = -1;
  if (!p) return 0;
  hipPointerAttribute_t attr;
  hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) { (void)hipGetLastError(); return 0; }
  if (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged) { if (dev) *dev = attr.device; return 1; }
  return 0;
}
static bool is_device_ptr(const void *p) { return ptr_location(p, nullptr) == 1; }

// device selection: env CUDA_DEVICE is honoured like the reference (cuda_utils.cu:187-247) but visibility variables
// need not be set; HIP_DEVICE takes precedence.
int select_device() {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    (void)hipGetLastError();
    set_error(10, "no HIP device available (hipGetDeviceCount: %s). This engine is GPU-only.", hipGetErrorString(e));
    return -1;
  }
  int cur = 0;
  (void)hipGetDevice(&cur);
  int dev = cur;
  const char *d = getenv("HIP_DEVICE");
  if (!d) d = getenv("CUDA_DEVICE");
  if (d) dev = atoi(d);
  if (dev < 0 || dev >= count) {
    set_error(11, "The requested device %d is not visible to the HIP runtime (%d devices).", dev, count);
    return -1;
  }
  if (!check_hip(hipSetDevice(dev), __func__, __LINE__)) return -1;
  return dev;
}

}  // namespace mxa

using namespace mxa;

// ================================================================================================ C ABI
extern "C" {

void setOptions_compressed(int use_gpu, int cores, int floatLoop, int meanSubstract, int ignore_missings, int do_not_center,
                           int do_normalize, int use_miraculix_freq, int variant, int print_details) {
  (void)cores; (void)floatLoop; (void)meanSubstract; (void)variant;
  if (print_details > 0 || env_print_level() > 0) printf("get started\n");  // the reference prints this unconditionally (5codesAPI.c:56)
  clear_error();
  if (!use_gpu) {
    // GPU-only engine.  The host process (a Julia / R session) must survive: report, remember, and let every later
    // plink2compressed leave its handle NULL (the Julia binding throws on a NULL handle, miraculix.jl:29-35).
    Options &o = options();
    o.gpu = false; o.set = true;
    set_error(14, "setOptions_compressed(use_gpu=0): this library is the MI355X engine only; the CPU 5codes engine is not part of "
                  "it. Objects cannot be created until setOptions_compressed is called with use_gpu=1; load the reference library "
                  "for CPU runs.");
    return;
  }
  // same fatal combination as the reference (5codesChar.cc:192-193, ERR0 -> fprintf(stderr)+exit)
  if (use_miraculix_freq || !ignore_missings || do_normalize) {
    fprintf(stderr, "in case of 'gpu' the Fortran frequency must always be used; missings/centering/normalizing cannot treated.\n");
    exit(EXIT_FAILURE);
  }
  Options &o = options();
  o.gpu = true;
  o.centered = !do_not_center;
  o.print_level = print_details;
  o.set = true;
}

void plink2compressed(char *plink, char *plink_transposed, int snps, int indiv, double *f, int max_n, void **compressed) {
  clear_error();
  const size_t ps = ((size_t)indiv + 3) / 4, pi = ((size_t)snps + 3) / 4;
  const int shards = multi_requested();
  if (shards > 1 || getenv("MXA_FORCE_MULTI")) {   // MIRACULIX_NUM_GPUS > 1: SNP blocks over several devices behind the same handle
    (void)multi_create(reinterpret_cast<const uint8_t *>(plink), reinterpret_cast<const uint8_t *>(plink_transposed), snps, indiv, f, max_n, shards, compressed);
    return;
  }
  (void)create_handle(reinterpret_cast<const uint8_t *>(plink), ps, reinterpret_cast<const uint8_t *>(plink_transposed), pi, snps, indiv, f,
                      max_n, compressed);
}

void mxa_plink2compressed_shard(char *plink, char *plink_transposed, int snps_total, int indiv, int snp_begin, int snp_end, double *f,
                                int max_n, void **compressed) {
  clear_error();
  if (compressed) *compressed = nullptr;
  if (snp_begin < 0 || snp_end > snps_total || snp_begin >= snp_end || (snp_begin & 3)) {
    set_error(1, "mxa_plink2compressed_shard: need 0 <= snp_begin < snp_end <= snps_total and snp_begin %% 4 == 0");
    return;
  }
  const size_t ps = ((size_t)indiv + 3) / 4, pi = ((size_t)snps_total + 3) / 4;
  const uint8_t *p = reinterpret_cast<const uint8_t *>(plink) + (size_t)snp_begin * ps;
  const uint8_t *pt = (!plink_transposed || plink_transposed == plink) ? nullptr : reinterpret_cast<const uint8_t *>(plink_transposed) + (size_t)snp_begin / 4;
  (void)create_handle(p, ps, pt, pi, snp_end - snp_begin, indiv, f ? f + snp_begin : nullptr, max_n, compressed);
}

int mxa_plink2compressed_begin(long snps, long indiv, int max_n, void **compressed) {
  clear_error();
  return begin_handle(snps, indiv, max_n, compressed);
}
int mxa_plink2compressed_rows(void *compressed, const unsigned char *plink_rows, long snp_begin, long nrows, const double *f_rows) {
  clear_error();
  if (is_multi(compressed)) { set_error(16, "mxa_plink2compressed_rows: not available on a multi-device object"); return 1; }
  Handle *h = as_handle(compressed, "mxa_plink2compressed_rows");
  return h ? append_rows(h, plink_rows, snp_begin, nrows, f_rows) : 1;
}
int mxa_plink2compressed_end(void *compressed) {
  clear_error();
  if (is_multi(compressed)) { set_error(16, "mxa_plink2compressed_end: not available on a multi-device object"); return 1; }
  Handle *h = as_handle(compressed, "mxa_plink2compressed_end");
  return h ? end_handle(h) : 1;
}

static int trans_flag(const char *trans) {  // 5codesAPI.c:73-77
  if (!trans) exit(99);   // the reference dereferences it; a NULL letter is "anything else"
  if (*trans == 'T' || *trans == 't' || *trans == 'Y' || *trans == 'y') return 1;
  if (*trans != 'N' && *trans != 'n') exit(99);
  return 0;
}

void dgemm_compressed(char *trans, void *compressed, int n, double *B, int Ldb, double *C, int Ldc) {
  clear_error();
  const int t = trans_flag(trans);
  if (is_multi(compressed)) { (void)multi_gemm(compressed, t != 0, n, B, Ldb, C, Ldc); return; }
  Handle *h = as_handle(compressed, "dgemm_compressed");
  if (!h) return;
  (void)gemm_any(h, t != 0, n, B, Ldb, C, Ldc, Ldc, true, true);
}

int mxa_dgemm_compressed_device(char trans, void *compressed, int n, const double *dB, long ldb, double *dC, long ldc, void *hip_stream,
                                int sync) {
  clear_error();
  const int t = trans_flag(&trans);
  if (is_multi(compressed)) { set_error(16, "mxa_dgemm_compressed_device: not available on a multi-device object (MIRACULIX_NUM_GPUS > 1); use dgemm_compressed or mxa_dgemm_compressed_multi"); return 1; }
  Handle *h = as_handle(compressed, "mxa_dgemm_compressed_device");
  if (!h) return 1;
  if (n <= 0) return 0;
  if (refuse_while_staging(h, "mxa_dgemm_compressed_device")) return 1;
  MXA_HIP(hipSetDevice(h->device));
  hipStream_t s = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : h->stream;
  if (gemm_device(h, t != 0, n, dB, ldb, dC, ldc, ldc, s, sync != 0)) return 1;
  if (sync) { MXA_HIP(hipStreamSynchronize(s)); harvest_profile(h); }
  return 0;
}

int mxa_gram_matvec(void *compressed, int n, const double *V, long ldv, double *out, long ldo) {
  clear_error();
  if (is_multi(compressed)) return multi_gram(compressed, n, V, ldv, out, ldo);
  Handle *h = as_handle(compressed, "mxa_gram_matvec");
  if (!h) return 1;
  return gram_any(h, n, V, ldv, out, ldo, true);
}

int mxa_gram_matvec_device(void *compressed, int n, const double *dV, long ldv, double *dOut, long ldo, int sync) {
  clear_error();
  if (is_multi(compressed)) { set_error(16, "mxa_gram_matvec_device: not available on a multi-device object; use mxa_gram_matvec"); return 1; }
  Handle *h = as_handle(compressed, "mxa_gram_matvec_device");
  if (!h) return 1;
  int vd = -1, od = -1;
  if (ptr_location(dV, &vd) != 1 || ptr_location(dOut, &od) != 1 || vd != h->device || od != h->device) {
    set_error(1, "mxa_gram_matvec_device: V and out must be memory of the object's device (%d)", h->device);
    return 1;
  }
  return gram_any(h, n, dV, ldv, dOut, ldo, sync != 0);
}

void free_compressed(void **compressed) {
  if (!compressed || !*compressed) return;
  if (is_multi(*compressed)) { multi_destroy(*compressed); *compressed = nullptr; return; }
  Handle *h = as_handle(*compressed, "free_compressed");
  if (h) destroy_handle(h);
  *compressed = nullptr;
}

// ------------------------------------------------------------------------------------------------ sparse x packed
namespace {
struct DevBuf {   // frees on scope exit
  void *p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  int alloc(size_t bytes) { MXA_HIP(hipMalloc(&p, bytes ? bytes : 1)); return 0; }
};
// size of one piece of the host staging, read per call: MXA_SPARSE_CHUNK_BYTES (the bounce buffer of the gathered packed rows, default 256 MiB) and
// MXA_SPARSE_SLAB_BYTES (the device buffer a host C leaves through, default 1 GiB).  A piece size changes how often the loops run, never a result.
size_t sparse_piece_bytes(const char *name, size_t dflt) {
  const char *e = getenv(name);
  return e && atoll(e) > 0 ? (size_t)atoll(e) : dflt;
}
}  // namespace

static int sparse_times_plink_impl(bool tcompressed, const uint8_t *plink, const uint8_t *plink_transposed, int snps, int indiv, int nIdx,
                                   const int *rowIdxB, const int *colIdxB, const double *B, double *C, long ldc) {
  // reference semantics, pinned by running its library (tests/golden/make_golden_sparse.py): the sparse column index selects a ROW of
  // the packed matrix, the result runs over the 2-bit entries of that row:
  //   'N': P = plink (snps rows of indiv entries):             C (nIdx x indiv) = S (nIdx x snps)  * Z^T
  //   'T': P = plink_transposed (indiv rows of snps entries):  C (nIdx x snps)  = S (nIdx x indiv) * Z
  // zero-based CSR, uncentred, missing -> 0, C zero-filled over Ldc x entries (haplogeno.cc:1696).
  const uint8_t *P = tcompressed ? plink_transposed : plink;
  const long rows = tcompressed ? indiv : snps, entries = tcompressed ? snps : indiv;
  if (!P || !rowIdxB || !C || snps <= 0 || indiv <= 0 || nIdx < 0) { set_error(1, "sparse_times_plink: invalid argument"); return 1; }
  if (ldc < nIdx) { set_error(7, "sparse_times_plink: Ldc %ld < nIdx %d", ldc, nIdx); return 1; }
  const int dev = select_device();
  if (dev < 0) return 1;
  if (nIdx == 0) {   // no sparse row: the zero-fill of Ldc x entries is all there is (the reference memsets before it looks at nIdx)
    const size_t bytes = sizeof(double) * (size_t)ldc * (size_t)entries;
    if (bytes && is_device_ptr(C)) {
      MXA_HIP(hipMemsetAsync(C, 0, bytes, nullptr));
      MXA_HIP(hipStreamSynchronize(nullptr));
    } else if (bytes) {
      memset(C, 0, bytes);
    }
    return 0;
  }
  const size_t pitch = ((size_t)entries + 3) / 4;
  // CSR arrays on the host for validation
  std::vector<int> h_row((size_t)nIdx + 1);
  MXA_HIP(hipMemcpy(h_row.data(), rowIdxB, sizeof(int) * ((size_t)nIdx + 1), is_device_ptr(rowIdxB) ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
  const long nnz = h_row[nIdx];
  if (h_row[0] != 0 || nnz < 0) { set_error(1, "sparse_times_plink: rowIdxB must be zero-based CSR row pointers (rowIdxB[0] = %d)", h_row[0]); return 1; }
  for (int j = 0; j < nIdx; j++) if (h_row[j + 1] < h_row[j]) { set_error(1, "sparse_times_plink: rowIdxB is not non-decreasing at row %d", j); return 1; }
  if (nnz > 0 && (!colIdxB || !B)) { set_error(1, "sparse_times_plink: colIdxB / B are NULL"); return 1; }
  std::vector<int> h_col((size_t)nnz);
  if (nnz) MXA_HIP(hipMemcpy(h_col.data(), colIdxB, sizeof(int) * (size_t)nnz, is_device_ptr(colIdxB) ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
  for (long t = 0; t < nnz; t++)
    if (h_col[t] < 0 || h_col[t] >= rows) { set_error(1, "sparse_times_plink: colIdxB[%ld] = %d outside [0, %ld)", t, h_col[t], rows); return 1; }

  // packed rows on the device: a device matrix is used in place; from the host only the rows S refers to are uploaded
  DevBuf dP;
  const uint8_t *d_packed = P;
  if (!is_device_ptr(P)) {
    std::vector<int> remap((size_t)rows, -1), used;
    for (long t = 0; t < nnz; t++) if (remap[h_col[t]] < 0) { remap[h_col[t]] = 0; used.push_back(h_col[t]); }
    std::sort(used.begin(), used.end());
    for (size_t u = 0; u < used.size(); u++) remap[used[u]] = (int)u;
    for (long t = 0; t < nnz; t++) h_col[t] = remap[h_col[t]];
    if (dP.alloc(used.size() * pitch)) return 1;
    const size_t rows_per_chunk = std::max<size_t>(1, sparse_piece_bytes("MXA_SPARSE_CHUNK_BYTES", (size_t)256 << 20) / pitch);
    debug_info("sparse_times_plink: %zu of %ld packed rows uploaded in %zu chunk(s) of at most %zu rows", used.size(), rows,
               (used.size() + rows_per_chunk - 1) / rows_per_chunk, rows_per_chunk);
    std::vector<uint8_t> bounce(std::min(rows_per_chunk, std::max<size_t>(1, used.size())) * pitch);
    for (size_t u0 = 0; u0 < used.size(); u0 += rows_per_chunk) {
      const size_t cnt = std::min(rows_per_chunk, used.size() - u0);
      for (size_t u = 0; u < cnt; u++) memcpy(bounce.data() + u * pitch, P + (size_t)used[u0 + u] * pitch, pitch);
      MXA_HIP(hipMemcpy(static_cast<uint8_t *>(dP.p) + u0 * pitch, bounce.data(), cnt * pitch, hipMemcpyHostToDevice));
    }
    d_packed = static_cast<const uint8_t *>(dP.p);
  }
  DevBuf dRow, dCol, dVal;
  if (dRow.alloc(sizeof(int) * ((size_t)nIdx + 1)) || dCol.alloc(sizeof(int) * (size_t)nnz) || dVal.alloc(sizeof(double) * (size_t)nnz)) return 1;
  MXA_HIP(hipMemcpy(dRow.p, h_row.data(), sizeof(int) * ((size_t)nIdx + 1), hipMemcpyHostToDevice));
  if (nnz) {
    MXA_HIP(hipMemcpy(dCol.p, h_col.data(), sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice));
    MXA_HIP(hipMemcpy(dVal.p, B, sizeof(double) * (size_t)nnz, is_device_ptr(B) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  }
  hipStream_t s = nullptr;   // legacy default stream: ordered with everything else of the process
  if (is_device_ptr(C)) {
    if (launch_sparse_times_plink(d_packed, pitch, entries, nIdx, (const int *)dRow.p, (const int *)dCol.p, (const double *)dVal.p, C, ldc, 0, entries, s)) return 1;
    MXA_HIP(hipStreamSynchronize(s));
    return 0;
  }
  // host C: slabs of columns (multiples of 512, at least 512) through a device buffer of at most 1 GiB or MXA_SPARSE_SLAB_BYTES
  long e_slab = std::max<long>(512, ((long)sparse_piece_bytes("MXA_SPARSE_SLAB_BYTES", (size_t)1 << 30) / (8 * ldc)) / 512 * 512);
  e_slab = std::min(e_slab, (entries + 511) / 512 * 512);
  debug_info("sparse_times_plink: host C in %ld slab(s) of at most %ld columns", (entries + e_slab - 1) / e_slab, e_slab);
  DevBuf dC;
  if (dC.alloc(sizeof(double) * (size_t)ldc * (size_t)std::min(e_slab, entries))) return 1;   // (the kernel stores no column at or beyond `entries`)
  for (long e0 = 0; e0 < entries; e0 += e_slab) {
    const long cnt = std::min(e_slab, entries - e0);
    if (launch_sparse_times_plink(d_packed, pitch, entries, nIdx, (const int *)dRow.p, (const int *)dCol.p, (const double *)dVal.p, (double *)dC.p, ldc, e0, cnt, s)) return 1;
    MXA_HIP(hipMemcpy(C + (size_t)e0 * ldc, dC.p, sizeof(double) * (size_t)ldc * (size_t)cnt, hipMemcpyDeviceToHost));
  }
  return 0;
}

void sparse_times_plink(char *transsparse, char *transcompressed, char *plink, char *plink_transposed, int snps, int indiv, int nIdx, int *rowIdxB,
                        int *colIdxB, double *B, double *C, int Ldc) {
  clear_error();
  const int tc = trans_flag(transcompressed);
  if (trans_flag(transsparse)) {   // reference: BUG -> "Severe error occured in function 'sparseTGeno'" + exit (haplogeno.cc:1698)
    fprintf(stderr, "miraculix_amd: sparse_times_plink: a transposed sparse matrix is not supported (nor by the reference)\n");
    exit(EXIT_FAILURE);
  }
  (void)sparse_times_plink_impl(tc != 0, reinterpret_cast<const uint8_t *>(plink), reinterpret_cast<const uint8_t *>(plink_transposed), snps, indiv, nIdx,
                                rowIdxB, colIdxB, B, C, Ldc);
}

// dgemm_plink (5codesAPI.c:112-130): the documented semantics as plink2compressed + dgemm_compressed + free_compressed; see the header (parity unpinned:
// the reference aborts unconditionally there).
void dgemm_plink(char *trans, char *plink, char *plink_transposed, int snps, int indiv, double *f, int n, double *B, int Ldb, double *C, int Ldc) {
  clear_error();
  const int t = trans_flag(trans);
  if (snps <= 0 || indiv <= 0 || n < 0) { set_error(1, "dgemm_plink: snps and indiv must be positive"); return; }
  if (n == 0) return;
  if (!plink && !plink_transposed) { set_error(1, "dgemm_plink: plink and plink_transposed are both NULL"); return; }
  if (select_device() < 0) return;
  const size_t bps = ((size_t)indiv + 3) / 4, bpi = ((size_t)snps + 3) / 4;
  DevBuf tmp;
  const uint8_t *p_snp = reinterpret_cast<const uint8_t *>(plink);
  if (!p_snp) {   // only the individual-major matrix was handed over ('N' in the reference's call shape): the SNP-major copy is made on the device
    DevBuf src;
    const uint8_t *pt = reinterpret_cast<const uint8_t *>(plink_transposed);
    if (!is_device_ptr(pt)) {
      if (src.alloc((size_t)indiv * bpi) || !check_hip(hipMemcpy(src.p, pt, (size_t)indiv * bpi, hipMemcpyHostToDevice), __func__, __LINE__)) return;
      pt = static_cast<const uint8_t *>(src.p);
    }
    if (tmp.alloc((size_t)snps * bps) || launch_transpose_2bit(pt, indiv, snps, static_cast<uint8_t *>(tmp.p), nullptr) ||
        !check_hip(hipDeviceSynchronize(), __func__, __LINE__)) return;
    p_snp = static_cast<const uint8_t *>(tmp.p);
  }
  Options &o = options();
  const Options saved = o;
  o.gpu = true; o.centered = f != nullptr; o.set = true;
  void *obj = nullptr;
  tl_single_override = 1;                 // one product: the SNP-major copy serves it whichever way
  tl_no_warmup = true;
  const int rc = create_handle(p_snp, bps, nullptr, bpi, snps, indiv, f, n, &obj);
  tl_single_override = -1; tl_no_warmup = false;
  if (!rc && obj) {
    Handle *h = reinterpret_cast<Handle *>(obj);
    (void)gemm_any(h, t != 0, n, B, Ldb, C, Ldc, Ldc, true, true);
    destroy_handle(h);
  }
  o = saved;
}

void get_compressed_freq(void *compressed, double *f) {
  clear_error();
  if (is_multi(compressed)) { if (f) multi_freq(compressed, f); return; }
  Handle *h = as_handle(compressed, "get_compressed_freq");
  if (!h || !f) return;
  if (refuse_while_staging(h, "get_compressed_freq")) return;   // the host copy of the frequencies is filled when the object is sealed
  memcpy(f, h->h_f, sizeof(double) * (size_t)h->snps);
}

int mxa_last_error(void) { return g_err; }
const char *mxa_last_error_string(void) { return g_errmsg; }

int mxa_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) { (void)hipGetLastError(); return -1; }
  return c;
}

int mxa_set_engine(int engine) {
  if (engine != 0 && engine != 1 && engine != 3 && engine != 4) return g_engine.load();
  return g_engine.exchange(engine);
}
int mxa_get_engine(void) { return g_engine.load(); }

void mxa_profile_reset(void) { profile() = Profile(); }
void mxa_profile_get(int *launches, double *total_ms) {
  if (launches) *launches = profile().launches;
  if (total_ms) *total_ms = profile().total_ms;
}
int mxa_last_path(void) {
  Geometry g;
  { std::lock_guard<std::mutex> lk(g_prof_mutex); g = last_geometry(); }
  if (g.path != 4) return g.path;
  // n <= 2 under the default engine: the route was chosen on the device; read the verdict now (the entries that use it are synchronous)
  int flag = 0, prev = 0;
  if (!g.d_flag) return 2;
  (void)hipGetDevice(&prev);
  if (hipSetDevice(g.flag_dev) != hipSuccess || hipMemcpy(&flag, g.d_flag, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); flag = 0; }
  (void)hipSetDevice(prev);
  return flag ? 3 : 2;
}
int mxa_last_range_fallback(void *compressed) {
  if (!compressed || is_multi(compressed)) return -1;
  Handle *h = as_handle(compressed, "mxa_last_range_fallback");
  if (!h || !h->ws.d_denflag) return -1;
  int flag = 0, prev = 0;
  (void)hipGetDevice(&prev);
  if (hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess ||
      hipMemcpy(&flag, h->ws.d_denflag, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); flag = -1; }
  (void)hipSetDevice(prev);
  return flag;
}
void mxa_last_geometry(long *m, long *k, int *n, int *splits, int *a_tile, int *c_tile) {
  const Geometry &g = last_geometry();
  if (m) *m = g.m; if (k) *k = g.k; if (n) *n = g.n; if (splits) *splits = g.splits; if (a_tile) *a_tile = g.a; if (c_tile) *c_tile = g.c;
}

long mxa_plan_partial_doubles(long m, long k, int n) {
  if (m <= 0 || k <= 0 || n <= 0) return 0;
  const GemmPlan p = plan_gemm(m, (k + kSlabK - 1) / kSlabK * kSlabK, n);
  return (long)p.splits * p.n_pad * p.m_pad;
}
int mxa_single_orientation(void *compressed) {
  if (!compressed) return -1;
  if (is_multi(compressed)) return multi_single(compressed);
  Handle *h = as_handle(compressed, "mxa_single_orientation");
  return h ? (h->single ? 1 : 0) : -1;
}
long mxa_partial_capacity(void *compressed) {
  if (!compressed || is_multi(compressed)) return -1;
  Handle *h = as_handle(compressed, "mxa_partial_capacity");
  return h ? (long)h->ws.cap_P : -1;
}

// ---- .bed staging owned by the library
static long count_lines(const char *path) {
  FILE *fh = fopen(path, "rb");
  if (!fh) return -1;
  long n = 0; int c, last = '\n';
  while ((c = fgetc(fh)) != EOF) { if (c == '\n') n++; last = c; }
  if (last != '\n') n++;
  fclose(fh);
  return n;
}

static std::string bed_base(const char *bed_path) {
  std::string base(bed_path);
  if (base.size() > 4 && base.compare(base.size() - 4, 4, ".bed") == 0) base.resize(base.size() - 4);
  return base;
}

}  // extern "C"
extern "C" {

static int bed_dims(const char *who, const std::string &base, int *snps, int *indiv) {
  if (*snps <= 0) *snps = (int)count_lines((base + ".bim").c_str());
  if (*indiv <= 0) *indiv = (int)count_lines((base + ".fam").c_str());
  if (*snps <= 0 || *indiv <= 0) { set_error(1, "%s: dimensions unknown (no .bim/.fam next to %s.bed)", who, base.c_str()); return 1; }
  return 0;
}

int mxa_bed2compressed(const char *bed_path, int snps, int indiv, int max_n, void **compressed, double *f_out, int *snps_out, int *indiv_out) {
  clear_error();
  if (compressed) *compressed = nullptr;
  if (!bed_path || !compressed) { set_error(1, "mxa_bed2compressed: bad arguments"); return 1; }
  const std::string base = bed_base(bed_path);
  if (bed_dims("mxa_bed2compressed", base, &snps, &indiv)) return 1;
  int rc;
  const int shards = multi_requested();
  if (shards > 1 || getenv("MXA_FORCE_MULTI")) rc = multi_create_from_bed(base.c_str(), snps, indiv, max_n, shards, compressed, f_out);
  else rc = bed_range_to_handle(base.c_str(), snps, indiv, 0, snps, max_n, -1, compressed, f_out);
  if (!rc) { if (snps_out) *snps_out = snps; if (indiv_out) *indiv_out = indiv; }
  return rc;
}

int mxa_bed2compressed_range(const char *bed_path, int snps, int indiv, int snp_begin, int snp_end, int max_n, void **compressed, double *f_out) {
  clear_error();
  if (compressed) *compressed = nullptr;
  if (!bed_path || !compressed) { set_error(1, "mxa_bed2compressed_range: bad arguments"); return 1; }
  const std::string base = bed_base(bed_path);
  if (bed_dims("mxa_bed2compressed_range", base, &snps, &indiv)) return 1;
  return bed_range_to_handle(base.c_str(), snps, indiv, snp_begin, snp_end, max_n, -1, compressed, f_out);
}

// ---- staging helpers
int mxa_transpose_2bit(const unsigned char *in, long rows, long cols, unsigned char *out) {
  clear_error();
  if (!in || !out || rows <= 0 || cols <= 0) { set_error(1, "mxa_transpose_2bit: bad arguments"); return 1; }
  if (select_device() < 0) return 1;
  const size_t nin = (size_t)rows * ((cols + 3) / 4), nout = (size_t)cols * ((rows + 3) / 4);
  const bool in_dev = is_device_ptr(in), out_dev = is_device_ptr(out);
  uint8_t *d_in = const_cast<uint8_t *>(in), *d_out = out;
  int rc = 0;
  if (!in_dev) { MXA_HIP(hipMalloc((void **)&d_in, nin)); if (!check_hip(hipMemcpy(d_in, in, nin, hipMemcpyHostToDevice), __func__, __LINE__)) rc = 1; }
  if (!out_dev && !rc) { if (!check_hip(hipMalloc((void **)&d_out, nout), __func__, __LINE__)) rc = 1; }
  if (!rc) rc = launch_transpose_2bit(d_in, rows, cols, d_out, nullptr);
  if (!rc && !check_hip(hipDeviceSynchronize(), __func__, __LINE__)) rc = 1;
  if (!rc && !out_dev && !check_hip(hipMemcpy(out, d_out, nout, hipMemcpyDeviceToHost), __func__, __LINE__)) rc = 1;
  if (!in_dev && d_in) (void)hipFree(d_in);
  if (!out_dev && d_out) (void)hipFree(d_out);
  return rc;
}

int mxa_allele_freq(const unsigned char *plink, long snps, long indiv, double *f) {
  clear_error();
  if (!plink || !f || snps <= 0 || indiv <= 0) { set_error(1, "mxa_allele_freq: bad arguments"); return 1; }
  if (select_device() < 0) return 1;
  const size_t nin = (size_t)snps * ((indiv + 3) / 4);
  const bool in_dev = is_device_ptr(plink), out_dev = is_device_ptr(f);
  uint8_t *d_in = const_cast<uint8_t *>(plink);
  double *d_f = f;
  int rc = 0;
  if (!in_dev) { MXA_HIP(hipMalloc((void **)&d_in, nin)); if (!check_hip(hipMemcpy(d_in, plink, nin, hipMemcpyHostToDevice), __func__, __LINE__)) rc = 1; }
  if (!out_dev && !rc) { if (!check_hip(hipMalloc((void **)&d_f, sizeof(double) * snps), __func__, __LINE__)) rc = 1; }
  if (!rc) rc = launch_allele_freq(d_in, snps, indiv, d_f, nullptr);
  if (!rc && !check_hip(hipDeviceSynchronize(), __func__, __LINE__)) rc = 1;
  if (!rc && !out_dev && !check_hip(hipMemcpy(f, d_f, sizeof(double) * snps, hipMemcpyDeviceToHost), __func__, __LINE__)) rc = 1;
  if (!in_dev && d_in) (void)hipFree(d_in);
  if (!out_dev && d_f) (void)hipFree(d_f);
  return rc;
}

}  // extern "C"
