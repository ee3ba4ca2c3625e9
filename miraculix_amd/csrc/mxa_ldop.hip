// mxa_ldop.hip -- the LD operator object: the window's values T staged once in device memory, then applied and ridge-solved there (last subsection).
//
// Creation runs the existing rows driver (ld_window_any / ld_pairwise_any of mxa_ldwindow.hip) into a device buffer of the upper ragged rows, so T is bit
// for bit what mxa_ld_window_rows(_pairwise) stores; k_ld_op_mirror turns them into the MIRRORED ragged rows: row j holds T[j, first[j] .. last[j]]
// contiguously at full[ptr[j] ..].  By symmetry T[i, j] = full[ptr[j] + i - first[j]], so a workgroup of 256 consecutive output rows i that sweeps j upwards
// reads 256 consecutive doubles per j (k_ld_op_apply): the object is streamed once per chunk of columns, X[j, .] is a wave-uniform load.
// The solve is conjugate gradients on that apply, every scalar of every column kept on the device.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <mutex>
#include <set>
#include <vector>
#include "../../include/miraculix_amd.h"
#include "mxa_internal.h"
#include "mxa_ldop_host.h"
#include "mxa_xprod.h"

namespace mxa {

namespace {
constexpr int kOpRows = 256;         // output rows per workgroup of the apply (one per thread)
constexpr int kOpMaxNC = 16;         // columns a thread keeps in registers
constexpr int kDotRows = 1024;       // rows per workgroup of the vector kernels: the partial count depends on snps alone
constexpr int kOpMaxSolveCols = 65535;     // a column of the solve is one gridDim.y of its vector kernels

struct LdOp {
  int device = 0;
  long snps = 0, entries = 0, mirrored = 0;
  double *d_full = nullptr;
  int *d_first = nullptr, *d_last = nullptr;
  long *d_ptr = nullptr, *d_rowptr = nullptr, *d_base = nullptr;   // base[j] = ptr[j] - first[j]
  double *d_xt = nullptr;            // snps x 16 doubles: the column chunk of an apply, packed row by row (k_ld_op_pack)
  hipStream_t stream = nullptr;
  int *d_flag = nullptr;             // the solve's "columns still running" word
  long bytes = 0;
};

std::mutex g_live_mutex;
std::set<void *> g_live;             // the handles that exist: a stale or foreign pointer is rejected without being read

LdOp *live_op(void *p) {
  if (!p) return nullptr;
  std::lock_guard<std::mutex> lock(g_live_mutex);
  return g_live.count(p) ? static_cast<LdOp *>(p) : nullptr;
}

struct DeviceGuard {                 // the object's device for the length of a call
  int prev = -1;
  int enter(int dev) {
    MXA_HIP(hipGetDevice(&prev));
    if (prev != dev) MXA_HIP(hipSetDevice(dev)); else prev = -1;
    return 0;
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

int need_device_bytes(const char *who, size_t need) {
  size_t free_b = 0, total_b = 0;
  MXA_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > free_b) { set_error(12, "%s: not enough device memory: required %zu MB, free %zu MB", who, need >> 20, free_b >> 20); return 1; }
  return 0;
}
}  // namespace

// ---- kernels
// Mirror: one workgroup per row j = blk0 + blockIdx.x of the mirrored layout (launch_in_block_chunks: snps workgroups of 256 threads pass 2^32 threads at 2^24
// SNPs).  k >= j comes from row j of the upper rows (coalesced), k < j from row k (a gather: one uncoalesced pass, run once per object; neighbouring rows j
// touch neighbouring addresses, so most of it is served by the L2).
__global__ void __launch_bounds__(256) k_ld_op_mirror(const double *__restrict__ upper, const long *__restrict__ rowptr, const long *__restrict__ ptr,
                                                       const int *__restrict__ first, const int *__restrict__ last, double *__restrict__ full, long blk0) {
  const int j = (int)(blk0 + blockIdx.x);
  const int f = first[j], l = last[j];
  const long dst = ptr[j] - f, up = rowptr[j] - j;
  for (int k = f + (int)threadIdx.x; k <= l; k += 256) full[dst + k] = k >= j ? upper[up + k] : upper[rowptr[k] + (j - k)];
}

// the upper ragged rows back out of the mirrored ones
__global__ void __launch_bounds__(256) k_ld_op_upper(const double *__restrict__ full, const long *__restrict__ rowptr, const long *__restrict__ ptr,
                                                      const int *__restrict__ first, const int *__restrict__ last, double *__restrict__ upper, long blk0) {
  const int j = (int)(blk0 + blockIdx.x);
  const long src = ptr[j] - first[j], up = rowptr[j] - j;
  for (int k = j + (int)threadIdx.x; k <= last[j]; k += 256) upper[up + k] = full[src + k];
}

// Pack: the chunk's columns row by row, xt[j NC + c] = X[j, min(c, nc - 1)], so that the NC values of one j are one aligned, wave-uniform load in the apply
// (columns beyond nc, in a partial chunk, repeat column nc - 1 and are never stored).
template <int NC>
struct alignas(8 * NC) LdOpXRow { double v[NC]; };

template <int NC>
__global__ void __launch_bounds__(256) k_ld_op_pack(const double *__restrict__ X, long ldx, int nc, int snps, LdOpXRow<NC> *__restrict__ xt) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= snps) return;
  LdOpXRow<NC> r;
#pragma unroll
  for (int c = 0; c < NC; c++) r.v[c] = X[(size_t)min(c, nc - 1) * (size_t)ldx + i];
  xt[i] = r;
}

// Apply: Y[i, c] = fma(shift, X[i, c], s), s = the fma chain over j = first[i] .. last[i] ascending from 0.0: acc = fma(T[i, j], X[j, c], acc).  The order is
// fixed by i and the window alone; every column has its own chain, so a column's bits do not depend on n or on the chunk it falls into.  Thread t owns row
// i0 + t and NC accumulators; the workgroup sweeps j over [first[i0], last[i0 + 255]], a thread takes part while first[i] <= j <= last[i] (elements outside
// the window are skipped, never multiplied).  base[j] = ptr[j] - first[j]: T[i, j] = full[base[j] + i].  U values of j are in flight at once.
template <int NC, int U>
__global__ void __launch_bounds__(256) k_ld_op_apply(const double *__restrict__ full, const long *__restrict__ base, const int *__restrict__ first,
                                                      const int *__restrict__ last, int snps, double shift, const LdOpXRow<NC> *__restrict__ xt, int nc,
                                                      double *__restrict__ Y, long ldy) {
  const int i0 = (int)blockIdx.x * kOpRows, i = i0 + (int)threadIdx.x;
  const bool live = i < snps;
  const int jlo = first[i0], jhi = last[min(i0 + kOpRows - 1, snps - 1)];
  const int fi = live ? first[i] : 1, li = live ? last[i] : 0;        // a thread beyond the last row has an empty window
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; c++) acc[c] = 0.0;
  int j = jlo;
  for (; j + U - 1 <= jhi; j += U) {
    long b[U];
#pragma unroll
    for (int u = 0; u < U; u++) b[u] = base[j + u];
    double t[U];
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      in[u] = j + u >= fi && j + u <= li;
      t[u] = in[u] ? full[b[u] + i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < U; u++)
      if (in[u]) {
        const LdOpXRow<NC> x = xt[j + u];
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] = fma(t[u], x.v[c], acc[c]);
      }
  }
  for (; j <= jhi; j++)
    if (j >= fi && j <= li) {
      const double t = full[base[j] + i];
      const LdOpXRow<NC> x = xt[j];
#pragma unroll
      for (int c = 0; c < NC; c++) acc[c] = fma(t, x.v[c], acc[c]);
    }
  if (live) {
    const LdOpXRow<NC> x = xt[i];
#pragma unroll
    for (int c = 0; c < NC; c++)
      if (c < nc) Y[(size_t)c * (size_t)ldy + i] = fma(shift, x.v[c], acc[c]);
  }
}

// the sum of the workgroup's 256 values in a fixed tree; the result is valid in thread 0
__device__ __forceinline__ double ld_op_block_sum(double s, double *sh) {
  sh[threadIdx.x] = s;
  for (int w = 128; w > 0; w >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
  }
  __syncthreads();
  return sh[0];
}
// the sum of part[0 .. nblk) by one workgroup: thread t adds t, t + 256, .. in index order, then the tree
__device__ __forceinline__ double ld_op_sum_partials(const double *__restrict__ part, int nblk, double *sh) {
  double s = 0.0;
  for (int b = (int)threadIdx.x; b < nblk; b += 256) s += part[b];
  const double r = ld_op_block_sum(s, sh);
  __syncthreads();
  return r;
}

// The conjugate-gradient state of column c: status -1 running, 0 converged, 2 breakdown (the host turns a -1 left after max_iter into 1).
struct LdOpCg {
  double *rr, *bb, *alpha, *beta, *relres;
  int *iters, *status;
};

// r = p = B, X = 0 (grid: row blocks x columns)
__global__ void __launch_bounds__(256) k_ld_op_cg_init(const double *__restrict__ B, long ldb, long snps, double *__restrict__ X, long ldx, double *__restrict__ r,
                                                        double *__restrict__ p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const size_t c = blockIdx.y;
  if (i >= snps) return;
  const double b = B[c * (size_t)ldb + i];
  r[c * (size_t)snps + i] = b;
  p[c * (size_t)snps + i] = b;
  X[c * (size_t)ldx + i] = 0.0;
}

// part[c nblk + block] = sum over the block's 1024 rows of a[i, c] b[i, c]: thread t takes rows t, t + 256, t + 512, t + 768 as an fma chain, then the tree.
// Only running columns (status -1).
__global__ void __launch_bounds__(256) k_ld_op_dot(const double *__restrict__ a, const double *__restrict__ b, long snps, const int *__restrict__ status,
                                                    double *__restrict__ part) {
  __shared__ double sh[256];
  const size_t c = blockIdx.y;
  if (status[c] != -1) return;
  const long base = (long)blockIdx.x * kDotRows;
  double s = 0.0;
  for (int q = 0; q < kDotRows / 256; q++) {
    const long i = base + q * 256 + (long)threadIdx.x;
    if (i < snps) s = fma(a[c * (size_t)snps + i], b[c * (size_t)snps + i], s);
  }
  s = ld_op_block_sum(s, sh);
  if (threadIdx.x == 0) part[c * gridDim.x + blockIdx.x] = s;
}

// One workgroup, the columns in index order.  mode 0: rr = bb = b.b, the test before the first iteration (b = 0: relres 0, converged with X = 0).
// mode 1: pAp -> alpha = rr / pAp, or breakdown when pAp is not > 0.  mode 2: the new r.r -> iters + 1, relres = sqrt(rr) / sqrt(bb), converged when
// relres <= tol, else beta = rr_new / rr.  *flag = the number of columns still running.
__global__ void __launch_bounds__(256) k_ld_op_cg_scalars(int mode, int n, int nblk, const double *__restrict__ part, LdOpCg cg, double tol, int *__restrict__ flag) {
  __shared__ double sh[256];
  int running = 0;
  for (int c = 0; c < n; c++) {
    if (mode != 0 && cg.status[c] != -1) continue;                   // uniform: every thread reads the same word
    const double s = ld_op_sum_partials(part + (size_t)c * nblk, nblk, sh);
    if (threadIdx.x == 0) {
      if (mode == 0) {
        cg.rr[c] = cg.bb[c] = s;
        cg.iters[c] = 0;
        cg.relres[c] = s == 0.0 ? 0.0 : 1.0;
        cg.status[c] = s == 0.0 ? 0 : -1;
      } else if (mode == 1) {
        if (s > 0.0) cg.alpha[c] = __ddiv_rn(cg.rr[c], s);
        else cg.status[c] = 2;
      } else {
        const double rel = __ddiv_rn(__dsqrt_rn(s), __dsqrt_rn(cg.bb[c]));
        cg.iters[c] += 1;
        cg.relres[c] = rel;
        if (rel <= tol) cg.status[c] = 0;
        else cg.beta[c] = __ddiv_rn(s, cg.rr[c]);
        cg.rr[c] = s;
      }
    }
    __syncthreads();
    if (cg.status[c] == -1) running++;
  }
  if (threadIdx.x == 0) *flag = running;
}

// x += alpha p, r -= alpha Ap, and the block's partial of the new r.r -- one pass over the four vectors
__global__ void __launch_bounds__(256) k_ld_op_cg_update(long snps, const LdOpCg cg, const double *__restrict__ p, const double *__restrict__ Ap,
                                                          double *__restrict__ X, long ldx, double *__restrict__ r, double *__restrict__ part) {
  __shared__ double sh[256];
  const size_t c = blockIdx.y;
  if (cg.status[c] != -1) return;
  const double a = cg.alpha[c];
  const long base = (long)blockIdx.x * kDotRows;
  double s = 0.0;
  for (int q = 0; q < kDotRows / 256; q++) {
    const long i = base + q * 256 + (long)threadIdx.x;
    if (i < snps) {
      const size_t k = c * (size_t)snps + i, kx = c * (size_t)ldx + i;
      X[kx] = fma(a, p[k], X[kx]);
      const double ri = fma(-a, Ap[k], r[k]);
      r[k] = ri;
      s = fma(ri, ri, s);
    }
  }
  s = ld_op_block_sum(s, sh);
  if (threadIdx.x == 0) part[c * gridDim.x + blockIdx.x] = s;
}

// p = r + beta p
__global__ void __launch_bounds__(256) k_ld_op_cg_direction(long snps, const LdOpCg cg, const double *__restrict__ r, double *__restrict__ p) {
  const size_t c = blockIdx.y;
  if (cg.status[c] != -1) return;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= snps) return;
  const size_t k = c * (size_t)snps + i;
  p[k] = fma(cg.beta[c], p[k], r[k]);
}

// ---- host side
namespace {
template <int NC, int U>
void launch_apply_chunk(const LdOp *o, double shift, const double *dX, long ldx, int nc, double *dY, long ldy) {
  const unsigned blocks = (unsigned)((o->snps + kOpRows - 1) / kOpRows);
  LdOpXRow<NC> *xt = reinterpret_cast<LdOpXRow<NC> *>(o->d_xt);
  hipLaunchKernelGGL((k_ld_op_pack<NC>), dim3(blocks), dim3(256), 0, o->stream, dX, ldx, nc, (int)o->snps, xt);
  hipLaunchKernelGGL((k_ld_op_apply<NC, U>), dim3(blocks), dim3(kOpRows), 0, o->stream, (const double *)o->d_full, (const long *)o->d_base, (const int *)o->d_first,
                     (const int *)o->d_last, (int)o->snps, shift, (const LdOpXRow<NC> *)xt, nc, dY, ldy);
}

// Y = shift X + T X on device operands, enqueued on the object's stream: chunks of 16 columns, the last chunk on the narrowest kernel that holds it
int apply_device(const LdOp *o, double shift, const double *dX, long ldx, int n, double *dY, long ldy) {
  for (int c0 = 0; c0 < n; c0 += kOpMaxNC) {
    const int nc = std::min(kOpMaxNC, n - c0);
    const double *x = dX + (size_t)c0 * (size_t)ldx;
    double *y = dY + (size_t)c0 * (size_t)ldy;
    if (nc == 1) launch_apply_chunk<1, 8>(o, shift, x, ldx, nc, y, ldy);
    else if (nc == 2) launch_apply_chunk<2, 8>(o, shift, x, ldx, nc, y, ldy);
    else if (nc <= 4) launch_apply_chunk<4, 4>(o, shift, x, ldx, nc, y, ldy);
    else if (nc <= 8) launch_apply_chunk<8, 4>(o, shift, x, ldx, nc, y, ldy);
    else launch_apply_chunk<16, 4>(o, shift, x, ldx, nc, y, ldy);
  }
  MXA_HIP(hipGetLastError());
  return 0;
}

// the byte ranges of two snps x n column-major operands intersect
bool operands_overlap(const double *a, long lda, const double *b, long ldb, long snps, int n) {
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + sizeof(double) * ((size_t)(n - 1) * (size_t)lda + (size_t)snps);
  const uintptr_t b0 = (uintptr_t)b, b1 = b0 + sizeof(double) * ((size_t)(n - 1) * (size_t)ldb + (size_t)snps);
  return a0 < b1 && b0 < a1;
}

// takes the upper rows (device, `entries` doubles, owned by `upper`) and the checked window; builds the object and releases the upper rows
int finish_create(const char *who, long snps, const std::vector<int> &h_last, XBuf &upper, void **out) {
  std::vector<int> h_first((size_t)snps);
  std::vector<long> h_rowptr((size_t)snps + 1), h_ptr((size_t)snps + 1);
  long mirrored = 0;
  const long entries = ldop_layout(snps, h_last.data(), h_first.data(), h_rowptr.data(), h_ptr.data(), &mirrored);
  if (need_device_bytes(who, (size_t)ldop_object_bytes(snps, mirrored))) return 1;
  XBuf full, first, last, ptr, rowptr, base, xt, flag;
  std::vector<long> h_base((size_t)snps);
  for (long j = 0; j < snps; j++) h_base[(size_t)j] = h_ptr[(size_t)j] - h_first[(size_t)j];
  if (full.alloc(sizeof(double) * (size_t)mirrored) || first.alloc(sizeof(int) * (size_t)snps) || last.alloc(sizeof(int) * (size_t)snps) ||
      ptr.alloc(sizeof(long) * ((size_t)snps + 1)) || rowptr.alloc(sizeof(long) * ((size_t)snps + 1)) || base.alloc(sizeof(long) * (size_t)snps) ||
      xt.alloc(sizeof(double) * kOpMaxNC * (size_t)snps) || flag.alloc(sizeof(int))) return 1;
  MXA_HIP(hipMemcpy(first.p, h_first.data(), sizeof(int) * (size_t)snps, hipMemcpyHostToDevice));
  MXA_HIP(hipMemcpy(last.p, h_last.data(), sizeof(int) * (size_t)snps, hipMemcpyHostToDevice));
  MXA_HIP(hipMemcpy(ptr.p, h_ptr.data(), sizeof(long) * ((size_t)snps + 1), hipMemcpyHostToDevice));
  MXA_HIP(hipMemcpy(rowptr.p, h_rowptr.data(), sizeof(long) * ((size_t)snps + 1), hipMemcpyHostToDevice));
  MXA_HIP(hipMemcpy(base.p, h_base.data(), sizeof(long) * (size_t)snps, hipMemcpyHostToDevice));
  hipStream_t s = nullptr;
  MXA_HIP(hipStreamCreateWithFlags(&s, hipStreamDefault));   // blocking: ordered against the caller's default-stream work
  launch_in_block_chunks(snps, [&](unsigned nb, long blk0) {
    hipLaunchKernelGGL(k_ld_op_mirror, dim3(nb), dim3(256), 0, s, (const double *)upper.p, (const long *)rowptr.p, (const long *)ptr.p, (const int *)first.p,
                       (const int *)last.p, (double *)full.p, blk0);
  });
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { (void)hipStreamDestroy(s); MXA_HIP(e); }
  upper.release();
  int dev = 0;
  e = hipGetDevice(&dev);
  if (e != hipSuccess) { (void)hipStreamDestroy(s); MXA_HIP(e); }
  LdOp *o = new LdOp;
  o->device = dev;
  o->snps = snps; o->entries = entries; o->mirrored = mirrored;
  o->d_full = (double *)full.p; o->d_first = (int *)first.p; o->d_last = (int *)last.p; o->d_ptr = (long *)ptr.p; o->d_rowptr = (long *)rowptr.p;
  o->d_base = (long *)base.p; o->d_xt = (double *)xt.p; o->d_flag = (int *)flag.p;
  full.p = first.p = last.p = ptr.p = rowptr.p = base.p = xt.p = flag.p = nullptr;
  o->stream = s;
  o->bytes = ldop_object_bytes(snps, mirrored);
  {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    g_live.insert(o);
  }
  *out = o;
  return 0;
}

// `last` (host or device pointer) on the host, checked
int fetch_last(const char *who, long snps, const int *last, std::vector<int> &h_last) {
  h_last.resize((size_t)snps);
  MXA_HIP(hipMemcpy(h_last.data(), last, sizeof(int) * (size_t)snps, hipMemcpyDefault));
  const long bad = ldop_check_last(snps, h_last.data());
  if (bad >= 0) { set_error(1, "%s: need i <= last[i] < snps, non-decreasing (last[%ld] = %d, snps %ld)", who, bad, h_last[(size_t)bad], snps); return 1; }
  return 0;
}

int create_any(const char *who, const unsigned char *plink, int snps, int indiv, const int *last, int kind, bool pairwise, int is_plink, const double *freq,
               void **out) {
  if (!out) { set_error(1, "%s: bad arguments", who); return 1; }
  *out = nullptr;
  if (!plink || !last || snps <= 0 || indiv <= 0) { set_error(1, "%s: bad arguments", who); return 1; }
  if (!pairwise && !freq) { set_error(1, "%s: allele frequencies are required", who); return 1; }
  if (kind != 0 && kind != 1) { set_error(1, "%s: kind must be 0 or 1", who); return 1; }
  // what the rows driver would reject is rejected before the memory pre-flight, so that error 12 never stands in for error 1
  if (snps >= kXFusedMaxRows) { set_error(1, "%s: at most %ld SNPs per call", who, kXFusedMaxRows - 1); return 1; }
  if (pairwise && indiv > kPwMaxIndiv) { set_error(1, "%s: at most %ld individuals per call (4 indiv^2 must stay below 2^53)", who, kPwMaxIndiv); return 1; }
  if (select_device() < 0) return 1;
  std::vector<int> h_last;
  if (fetch_last(who, snps, last, h_last)) return 1;
  long mirrored = 0;
  const long entries = ldop_layout(snps, h_last.data(), nullptr, nullptr, nullptr, &mirrored);
  // the peak of the creation: the upper rows next to the mirrored ones (the rows driver checks its own staging against what is free once the upper rows stand)
  if (need_device_bytes(who, sizeof(double) * (size_t)entries + (size_t)ldop_object_bytes(snps, mirrored))) return 1;
  XBuf upper;
  if (upper.alloc(sizeof(double) * (size_t)entries)) return 1;
  const int rc = pairwise ? ld_pairwise_any(who, plink, snps, indiv, 0, last, (double *)upper.p, 0, false, kind)
                          : ld_window_any(who, plink, snps, indiv, 0, last, (double *)upper.p, 0, false, kind, is_plink != 0, freq);
  if (rc) return 1;
  return finish_create(who, snps, h_last, upper, out);
}

// the checks every call on an object shares; returns the object or nullptr (error set)
LdOp *enter(const char *who, void *op) {
  LdOp *o = live_op(op);
  if (!o) { set_error(1, "%s: not a live LD operator object", who); return nullptr; }
  return o;
}
}  // namespace

}  // namespace mxa

extern "C" int mxa_ld_op_bytes(int snps, const int *last, long *entries, long *bytes) {
  mxa::clear_error();
  const char *who = "mxa_ld_op_bytes";
  if (snps <= 0 || !last || !entries || !bytes) { mxa::set_error(1, "%s: bad arguments", who); return 1; }
  const long bad = mxa::ldop_check_last(snps, last);
  if (bad >= 0) { mxa::set_error(1, "%s: need i <= last[i] < snps, non-decreasing (last[%ld] = %d, snps %d)", who, bad, last[bad], snps); return 1; }
  long mirrored = 0;
  *entries = mxa::ldop_layout(snps, last, nullptr, nullptr, nullptr, &mirrored);
  *bytes = mxa::ldop_object_bytes(snps, mirrored);
  return 0;
}

extern "C" int mxa_ld_op_create(const unsigned char *plink, int snps, int indiv, const int *last, int kind, int is_plink_format, const double *allele_freq,
                                void **op) {
  mxa::clear_error();
  return mxa::create_any("mxa_ld_op_create", plink, snps, indiv, last, kind, false, is_plink_format, allele_freq, op);
}

extern "C" int mxa_ld_op_create_pairwise(const unsigned char *plink, int snps, int indiv, const int *last, int kind, void **op) {
  mxa::clear_error();
  return mxa::create_any("mxa_ld_op_create_pairwise", plink, snps, indiv, last, kind, true, 1, nullptr, op);
}

extern "C" int mxa_ld_op_from_rows(int snps, const int *last, const double *rows, void **op) {
  using namespace mxa;
  clear_error();
  const char *who = "mxa_ld_op_from_rows";
  if (!op) { set_error(1, "%s: bad arguments", who); return 1; }
  *op = nullptr;
  if (snps <= 0 || !last || !rows) { set_error(1, "%s: bad arguments", who); return 1; }
  if (snps >= kXFusedMaxRows) { set_error(1, "%s: at most %ld SNPs per call", who, kXFusedMaxRows - 1); return 1; }
  if (select_device() < 0) return 1;
  std::vector<int> h_last;
  if (fetch_last(who, snps, last, h_last)) return 1;
  long mirrored = 0;
  const long entries = ldop_layout(snps, h_last.data(), nullptr, nullptr, nullptr, &mirrored);
  if (need_device_bytes(who, sizeof(double) * (size_t)entries + (size_t)ldop_object_bytes(snps, mirrored))) return 1;
  XBuf upper;
  if (upper.alloc(sizeof(double) * (size_t)entries)) return 1;
  MXA_HIP(hipMemcpy(upper.p, rows, sizeof(double) * (size_t)entries, hipMemcpyDefault));
  return finish_create(who, snps, h_last, upper, op);
}

extern "C" int mxa_ld_op_rows(void *op, double *rows) {
  using namespace mxa;
  clear_error();
  const char *who = "mxa_ld_op_rows";
  LdOp *o = enter(who, op);
  if (!o) return 1;
  if (!rows) { set_error(1, "%s: bad arguments", who); return 1; }
  DeviceGuard dg;
  if (dg.enter(o->device)) return 1;
  const bool dev = ptr_location(rows, nullptr) == 1;
  XBuf tmp;
  const size_t bytes = sizeof(double) * (size_t)o->entries;
  if (!dev && (need_device_bytes(who, bytes) || tmp.alloc(bytes))) return 1;
  double *d = dev ? rows : (double *)tmp.p;
  launch_in_block_chunks(o->snps, [&](unsigned nb, long blk0) {
    hipLaunchKernelGGL(k_ld_op_upper, dim3(nb), dim3(256), 0, o->stream, (const double *)o->d_full, (const long *)o->d_rowptr, (const long *)o->d_ptr,
                       (const int *)o->d_first, (const int *)o->d_last, d, blk0);
  });
  MXA_HIP(hipGetLastError());
  if (!dev) MXA_HIP(hipMemcpyAsync(rows, d, bytes, hipMemcpyDeviceToHost, o->stream));
  MXA_HIP(hipStreamSynchronize(o->stream));
  return 0;
}

extern "C" int mxa_ld_op_apply(void *op, double shift, const double *X, long ldx, int n, double *Y, long ldy) {
  using namespace mxa;
  clear_error();
  const char *who = "mxa_ld_op_apply";
  LdOp *o = enter(who, op);
  if (!o) return 1;
  const long snps = o->snps;
  if (!X || !Y || n < 1) { set_error(1, "%s: bad arguments", who); return 1; }
  if (ldx < snps || ldy < snps) { set_error(1, "%s: need ldx >= snps and ldy >= snps (ldx %ld, ldy %ld, snps %ld)", who, ldx, ldy, snps); return 1; }
  if (!std::isfinite(shift)) { set_error(1, "%s: shift must be finite", who); return 1; }
  DeviceGuard dg;
  if (dg.enter(o->device)) return 1;
  const bool x_dev = ptr_location(X, nullptr) == 1, y_dev = ptr_location(Y, nullptr) == 1;
  if (x_dev == y_dev && operands_overlap(X, ldx, Y, ldy, snps, n)) { set_error(1, "%s: X and Y must not overlap", who); return 1; }
  const size_t cbytes = sizeof(double) * (size_t)snps * (size_t)n;       // a host operand's compact device copy (leading dimension snps)
  if (need_device_bytes(who, (x_dev ? 0 : cbytes) + (y_dev ? 0 : cbytes))) return 1;
  XBuf bx, by;
  if ((!x_dev && bx.alloc(cbytes)) || (!y_dev && by.alloc(cbytes))) return 1;
  const size_t col = sizeof(double) * (size_t)snps;
  if (!x_dev) MXA_HIP(hipMemcpy2DAsync(bx.p, col, X, sizeof(double) * (size_t)ldx, col, (size_t)n, hipMemcpyHostToDevice, o->stream));
  const double *dX = x_dev ? X : (const double *)bx.p;
  double *dY = y_dev ? Y : (double *)by.p;
  if (apply_device(o, shift, dX, x_dev ? ldx : snps, n, dY, y_dev ? ldy : snps)) return 1;
  if (!y_dev) MXA_HIP(hipMemcpy2DAsync(Y, sizeof(double) * (size_t)ldy, by.p, col, col, (size_t)n, hipMemcpyDeviceToHost, o->stream));
  MXA_HIP(hipStreamSynchronize(o->stream));
  return 0;
}

extern "C" int mxa_ld_op_solve(void *op, double shift, const double *B, long ldb, int n, double *X, long ldx, double tol, int max_iter, int *iters, double *relres,
                               int *status) {
  using namespace mxa;
  clear_error();
  const char *who = "mxa_ld_op_solve";
  LdOp *o = enter(who, op);
  if (!o) return 1;
  const long snps = o->snps;
  if (!B || !X || n < 1) { set_error(1, "%s: bad arguments", who); return 1; }
  if (n > kOpMaxSolveCols) { set_error(1, "%s: at most %d right-hand sides per call (n %d)", who, kOpMaxSolveCols, n); return 1; }
  if (ldb < snps || ldx < snps) { set_error(1, "%s: need ldb >= snps and ldx >= snps (ldb %ld, ldx %ld, snps %ld)", who, ldb, ldx, snps); return 1; }
  if (!std::isfinite(shift)) { set_error(1, "%s: shift must be finite", who); return 1; }
  if (!(tol > 0.0 && tol < 1.0)) { set_error(1, "%s: tol must lie in (0, 1)", who); return 1; }
  if (max_iter < 0) { set_error(1, "%s: max_iter must not be negative", who); return 1; }
  DeviceGuard dg;
  if (dg.enter(o->device)) return 1;
  const bool b_dev = ptr_location(B, nullptr) == 1, x_dev = ptr_location(X, nullptr) == 1;
  if (b_dev == x_dev && operands_overlap(B, ldb, X, ldx, snps, n)) { set_error(1, "%s: B and X must not overlap", who); return 1; }
  // workspace: r, p, Ap, device copies of a host B / X, the partial sums, the per-column scalars
  const size_t cbytes = sizeof(double) * (size_t)snps * (size_t)n;
  const int nblk = (int)((snps + kDotRows - 1) / kDotRows);
  const size_t pbytes = sizeof(double) * (size_t)nblk * (size_t)n, sbytes = (5 * sizeof(double) + 2 * sizeof(int)) * (size_t)n;
  if (need_device_bytes(who, (3 + (b_dev ? 0 : 1) + (x_dev ? 0 : 1)) * cbytes + pbytes + sbytes)) return 1;
  XBuf w_r, w_p, w_Ap, w_B, w_X, w_part, w_s;
  if (w_r.alloc(cbytes) || w_p.alloc(cbytes) || w_Ap.alloc(cbytes) || (!b_dev && w_B.alloc(cbytes)) || (!x_dev && w_X.alloc(cbytes)) || w_part.alloc(pbytes) ||
      w_s.alloc(sbytes)) return 1;
  hipStream_t s = o->stream;
  const size_t col = sizeof(double) * (size_t)snps;
  if (!b_dev) MXA_HIP(hipMemcpy2DAsync(w_B.p, col, B, sizeof(double) * (size_t)ldb, col, (size_t)n, hipMemcpyHostToDevice, s));
  const double *dB = b_dev ? B : (const double *)w_B.p;
  const long dldb = b_dev ? ldb : snps, dldx = x_dev ? ldx : snps;
  double *dX = x_dev ? X : (double *)w_X.p;
  double *r = (double *)w_r.p, *p = (double *)w_p.p, *Ap = (double *)w_Ap.p, *part = (double *)w_part.p;
  LdOpCg cg;
  cg.rr = (double *)w_s.p; cg.bb = cg.rr + n; cg.alpha = cg.bb + n; cg.beta = cg.alpha + n; cg.relres = cg.beta + n;
  cg.iters = (int *)(cg.relres + n); cg.status = cg.iters + n;
  MXA_HIP(hipMemsetAsync(cg.status, 0xff, sizeof(int) * (size_t)n, s));    // -1: running
  const dim3 g256((unsigned)((snps + 255) / 256), (unsigned)n), gdot((unsigned)nblk, (unsigned)n);
  int running = 0;
  auto read_flag = [&]() -> int {   // the one word the host waits for per iteration
    MXA_HIP(hipMemcpyAsync(&running, o->d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    MXA_HIP(hipStreamSynchronize(s));
    return 0;
  };
  hipLaunchKernelGGL(k_ld_op_cg_init, g256, dim3(256), 0, s, dB, dldb, snps, dX, dldx, r, p);
  hipLaunchKernelGGL(k_ld_op_dot, gdot, dim3(256), 0, s, (const double *)r, (const double *)r, snps, (const int *)cg.status, part);
  hipLaunchKernelGGL(k_ld_op_cg_scalars, dim3(1), dim3(256), 0, s, 0, n, nblk, (const double *)part, cg, tol, o->d_flag);
  MXA_HIP(hipGetLastError());
  if (read_flag()) return 1;
  for (int it = 0; it < max_iter && running > 0; it++) {
    if (apply_device(o, shift, p, snps, n, Ap, snps)) return 1;
    hipLaunchKernelGGL(k_ld_op_dot, gdot, dim3(256), 0, s, (const double *)p, (const double *)Ap, snps, (const int *)cg.status, part);
    hipLaunchKernelGGL(k_ld_op_cg_scalars, dim3(1), dim3(256), 0, s, 1, n, nblk, (const double *)part, cg, tol, o->d_flag);
    hipLaunchKernelGGL(k_ld_op_cg_update, gdot, dim3(256), 0, s, snps, cg, (const double *)p, (const double *)Ap, dX, dldx, r, part);
    hipLaunchKernelGGL(k_ld_op_cg_scalars, dim3(1), dim3(256), 0, s, 2, n, nblk, (const double *)part, cg, tol, o->d_flag);
    hipLaunchKernelGGL(k_ld_op_cg_direction, g256, dim3(256), 0, s, snps, cg, (const double *)r, p);
    MXA_HIP(hipGetLastError());
    if (read_flag()) return 1;
  }
  std::vector<double> h_rel((size_t)n);
  std::vector<int> h_it((size_t)n), h_st((size_t)n);
  MXA_HIP(hipMemcpyAsync(h_rel.data(), cg.relres, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
  MXA_HIP(hipMemcpyAsync(h_it.data(), cg.iters, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, s));
  MXA_HIP(hipMemcpyAsync(h_st.data(), cg.status, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, s));
  if (!x_dev) MXA_HIP(hipMemcpy2DAsync(X, sizeof(double) * (size_t)ldx, w_X.p, col, col, (size_t)n, hipMemcpyDeviceToHost, s));
  MXA_HIP(hipStreamSynchronize(s));
  for (int c = 0; c < n; c++) {
    if (iters) iters[c] = h_it[(size_t)c];
    if (relres) relres[c] = h_rel[(size_t)c];
    if (status) status[c] = h_st[(size_t)c] == -1 ? 1 : h_st[(size_t)c];
  }
  return 0;
}

extern "C" void mxa_ld_op_free(void **op) {
  using namespace mxa;
  if (!op || !*op) return;
  LdOp *o = nullptr;
  {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    auto it = g_live.find(*op);
    if (it != g_live.end()) { o = static_cast<LdOp *>(*op); g_live.erase(it); }
  }
  *op = nullptr;
  if (!o) return;                    // freed before, or never one of ours
  DeviceGuard dg;
  (void)dg.enter(o->device);
  if (o->stream) { (void)hipStreamSynchronize(o->stream); (void)hipStreamDestroy(o->stream); }
  (void)hipFree(o->d_full); (void)hipFree(o->d_first); (void)hipFree(o->d_last); (void)hipFree(o->d_ptr); (void)hipFree(o->d_rowptr); (void)hipFree(o->d_base);
  (void)hipFree(o->d_xt); (void)hipFree(o->d_flag);
  delete o;
}
