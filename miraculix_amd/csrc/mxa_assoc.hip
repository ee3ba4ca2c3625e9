// mxa_assoc.hip -- the association scan: per-SNP linear regression y_c ~ 1 + Q + x_s on packed genotypes (include/miraculix_amd.h: mxa_assoc_linear; DESIGN.md
// 3.6e).  The fp64 product does the work: D = Z^T B for B = [Y~ | Q] is the library's own uncentred 'T' product on a one-shot object.  What the product cannot
// know -- the missing calls -- comes from ONE streaming pass over the raw PLINK rows (k_assoc_scan): the exact counts N, c1, c2 of every SNP by popcount, and
// M_b = the sum of b over the SNP's missing individuals.  k_assoc_finish turns D, M and the counts into beta, se and t in the documented operation order.
// The score test for binary traits (mxa_assoc_score) is the same scan with B = [R | Wt | H] and one more sum per weight column, E = the weights
// summed over the SNP's 11 fields (k_assoc_weights, dense); k_assoc_score_finish is its epilogue.  Its null model is host code: mxa_assoc_null_host.h.
// A stage of another unit may follow that epilogue on the scan's stream and buffers, through assoc_score_then (mxa_assoc_stage.h): the saddlepoint correction
// and the fit of the effect sizes in mxa_assoc_spa.hip, the set tests in mxa_assoc_set.hip.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <new>
#include "../../include/miraculix_amd.h"
#include "mxa_internal.h"
#include "mxa_assoc_host.h"
#include "mxa_assoc_null_host.h"
#include "mxa_assoc_stage.h"
#include "mxa_xprod.h"

namespace mxa {

namespace {

struct alignas(8 * kAssocCols) AssocRow { double v[kAssocCols]; };   // one individual's 16 columns of B: one aligned 128-byte run

// ---- the sums of the phenotype preparation: 256 threads, thread t takes the individuals t, t + 256, ... in ascending order, then the fixed tree of
// assoc_block_sums (mxa_assoc_stage.h).  The order depends on indiv alone.
// out[x + y ld_out] = sum_i A[i, a] B[i, y] with a = x (diag == 0) or a = y (diag != 0: the squared norms, launched with gridDim.x == 1); A == nullptr: the
// column sums of B.  One workgroup per output.
__global__ void __launch_bounds__(256) k_assoc_dots(const double *__restrict__ A, long lda, const double *__restrict__ B, long ldb, long indiv,
                                                     double *__restrict__ out, int ld_out, int diag) {
  __shared__ double red[1][4];
  const double *b = B + (size_t)blockIdx.y * (size_t)ldb;
  const double *a = A ? A + (size_t)(diag ? blockIdx.y : blockIdx.x) * (size_t)lda : nullptr;
  double acc[1] = {0.0};
  for (long i = threadIdx.x; i < indiv; i += 256) acc[0] = a ? __fma_rn(a[i], b[i], acc[0]) : acc[0] + b[i];
  assoc_block_sums<1>(acc, red);
  if (threadIdx.x == 0) out[(size_t)blockIdx.x + (size_t)blockIdx.y * (size_t)ld_out] = acc[0];
}

// y[i, c] -= sum[c] / indiv
__global__ void __launch_bounds__(256) k_assoc_center(double *__restrict__ Y, long ldy, long indiv, const double *__restrict__ sum) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= indiv) return;
  const double mean = __ddiv_rn(sum[blockIdx.y], (double)indiv);
  double *y = Y + (size_t)blockIdx.y * (size_t)ldy;
  y[i] = __dsub_rn(y[i], mean);
}

// y[i, c] <- y[i, c] - sum_q Q[i, q] a[q, c]: the chain y = fma(-a[q, c], Q[i, q], y) over ascending q
__global__ void __launch_bounds__(256) k_assoc_project(double *__restrict__ Y, long ldy, long indiv, const double *__restrict__ Q, long ldq, int k,
                                                        const double *__restrict__ a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= indiv) return;
  double *y = Y + (size_t)blockIdx.y * (size_t)ldy;
  double v = y[i];
  for (int q = 0; q < k; q++) v = __fma_rn(-a[q + (size_t)blockIdx.y * k], Q[(size_t)q * (size_t)ldq + i], v);
  y[i] = v;
}

// the row-packed copy of B: chunk cc = blockIdx.y holds the columns [16 cc, 16 cc + 16) of every individual as one AssocRow (columns beyond ncols: zeros),
// as k_ld_op_pack does for X
__global__ void __launch_bounds__(256) k_assoc_pack(const double *__restrict__ B, long ldb, int ncols, long indiv, AssocRow *__restrict__ bp) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= indiv) return;
  const int c0 = (int)blockIdx.y * kAssocCols;
  AssocRow r;
#pragma unroll
  for (int c = 0; c < kAssocCols; c++) r.v[c] = c0 + c < ncols ? B[(size_t)(c0 + c) * (size_t)ldb + i] : 0.0;
  bp[(size_t)blockIdx.y * (size_t)indiv + i] = r;
}

// ---- the scan: one workgroup per SNP row blk0 + blockIdx.x of `rows` (compact pitch bps = ceil(indiv / 4)).  The row is cut into logical words of 16 bytes
// = 64 genotypes, counted from the row's first byte; thread t takes the words t, t + 256, ... in ascending order, two in flight.  Every word is read with
// 16-byte loads whatever the row's address: a row that starts `sh` bytes behind a 16-byte boundary takes the two aligned words its logical word lies in and
// shifts them together (assoc_load_word) -- the same logical word, so the same sums, for every alignment.  Fields at and beyond indiv are
// masked to 00 (N counts what is left: indiv - #01).  With H = (w >> 1) & 0x55.., L = w & 0x55..: 01 = L & ~H, 10 = H & ~L, 11 = H & L, counted by popcount;
// for every 01 field the individual's packed row of B is added to the thread's 16 accumulators, ascending individual.  Reduction: the wave's shuffles, then
// (w0 + w1) + (w2 + w3) through the LDS: nothing in the order depends on the data or the launch.  A row without any 01 stores zeros without reducing (the
// sum of zeros).  first != 0: this launch also stores the counts.  *flag is raised when a 01 was seen.
// (AssocWord and assoc_load_word, the logical word of a row: mxa_assoc_stage.h)

__device__ __forceinline__ void assoc_half(unsigned long long x, long fbase, long indiv, const AssocRow *__restrict__ bp, double (&acc)[kAssocCols], int &n01, int &n10,
                                           int &n11) {
  const long valid = indiv - fbase;
  if (valid <= 0) return;
  if (valid < 32) x &= (1ull << (2 * valid)) - 1ull;
  const unsigned long long L = x & 0x5555555555555555ull, H = (x >> 1) & 0x5555555555555555ull;
  unsigned long long miss = L & ~H;
  n01 += __popcll(miss);
  n10 += __popcll(H & ~L);
  n11 += __popcll(H & L);
  while (miss) {
    const int bit = __ffsll((long long)miss) - 1;
    const double2 *p = reinterpret_cast<const double2 *>(bp + (fbase + (bit >> 1)));
#pragma unroll
    for (int j = 0; j < kAssocCols / 2; j++) { const double2 v = p[j]; acc[2 * j] += v.x; acc[2 * j + 1] += v.y; }
    miss &= miss - 1ull;
  }
}

__global__ void __launch_bounds__(256) k_assoc_scan(const uint8_t *__restrict__ rows, long bps, long indiv, long row0, const AssocRow *__restrict__ bp, int c0,
                                                     int ncols, double *__restrict__ M, long ldm, int *__restrict__ nobs, int *__restrict__ c1,
                                                     int *__restrict__ c2, int first, int *__restrict__ flag, long blk0) {
  __shared__ double red[4][kAssocCols];
  __shared__ int redi[4][3];
  const long r = blk0 + blockIdx.x;
  const uint8_t *row = rows + (size_t)r * (size_t)bps;
  const int sh = (int)(reinterpret_cast<uintptr_t>(row) & 15);
  const long nwords = (bps + 15) / 16;
  double acc[kAssocCols];
#pragma unroll
  for (int j = 0; j < kAssocCols; j++) acc[j] = 0.0;
  int n01 = 0, n10 = 0, n11 = 0;
  for (long w = threadIdx.x; w < nwords; w += 512) {
    const AssocWord a = assoc_load_word(row, w, bps, sh);
    AssocWord b = {0ull, 0ull};
    if (w + 256 < nwords) b = assoc_load_word(row, w + 256, bps, sh);
    assoc_half(a.lo, 64 * w, indiv, bp, acc, n01, n10, n11);
    assoc_half(a.hi, 64 * w + 32, indiv, bp, acc, n01, n10, n11);
    assoc_half(b.lo, 64 * (w + 256), indiv, bp, acc, n01, n10, n11);
    assoc_half(b.hi, 64 * (w + 256) + 32, indiv, bp, acc, n01, n10, n11);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int any = __syncthreads_or(n01 != 0);
  if (first) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { n01 += __shfl_down(n01, off, 64); n10 += __shfl_down(n10, off, 64); n11 += __shfl_down(n11, off, 64); }
    if (lane == 0) { redi[wave][0] = n01; redi[wave][1] = n10; redi[wave][2] = n11; }
  }
  if (any) {
#pragma unroll
    for (int j = 0; j < kAssocCols; j++) {
      double v = acc[j];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
      if (lane == 0) red[wave][j] = v;
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < kAssocCols && c0 + t < ncols) M[(size_t)(c0 + t) * (size_t)ldm + (size_t)(row0 + r)] = any ? (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]) : 0.0;
  if (first && t >= 64 && t < 67) {
    const int q = t - 64, s = (redi[0][q] + redi[1][q]) + (redi[2][q] + redi[3][q]);
    if (q == 0) nobs[row0 + r] = (int)indiv - s;
    else if (q == 1) c1[row0 + r] = s;
    else c2[row0 + r] = s;
  }
  if (any && t == 128) *flag = 1;
}

// ---- the epilogue: one thread per (SNP, phenotype), every operation rounded once in the header's order
__global__ void __launch_bounds__(256) k_assoc_finish(long snps, int n, int k, const int *__restrict__ nobs, const int *__restrict__ c1, const int *__restrict__ c2,
                                                       const double *__restrict__ D, const double *__restrict__ M, long ld, const double *__restrict__ T,
                                                       const double *__restrict__ syy, double dof, double *__restrict__ beta, double *__restrict__ se,
                                                       double *__restrict__ tstat, long ldo, long blk0) {
  const long idx = (blk0 + blockIdx.x) * 256 + threadIdx.x;
  if (idx >= snps * (long)n) return;
  const long s = idx % snps;
  const int c = (int)(idx / snps);
  const long N = nobs[s], a1 = c1[s], a2 = c2[s];
  const long Sz = a1 + 2 * a2, Szz = a1 + 4 * a2;
  const double dN = (double)N;
  const double mu = __ddiv_rn((double)Sz, dN);
  const double v0 = __ddiv_rn((double)(N * Szz - Sz * Sz), dN);
  double sxx = v0;
  for (int q = 0; q < k; q++) {
    const size_t at = (size_t)s + (size_t)(n + q) * (size_t)ld;
    const double g = __fma_rn(mu, __dsub_rn(M[at], T[n + q]), D[at]);
    sxx = __fma_rn(-g, g, sxx);
  }
  const size_t at = (size_t)s + (size_t)c * (size_t)ld;
  const double g = __fma_rn(mu, __dsub_rn(M[at], T[c]), D[at]);
  const double b = __ddiv_rn(g, sxx);
  const double rss = __fma_rn(-b, g, syy[c]);
  const double e = __dsqrt_rn(__ddiv_rn(__ddiv_rn(rss, dof), sxx));
  const size_t o = (size_t)s + (size_t)c * (size_t)ldo;
  if (beta) beta[o] = b;
  if (se) se[o] = e;
  if (tstat) tstat[o] = __ddiv_rn(b, e);
}

// ---- the score test's one new sum: E[r, c] = sum over the individuals with code 11 in row r of w_c.  Dense, not a gather (11 fields are 10-25 % of all
// fields): a workgroup takes kScoreRows SNP rows and C = kScoreCols weight columns (further columns: further passes).  Thread t owns the individuals of the
// logical words t, t + 256, ... (the words of assoc_load_word, so every alignment gives the same sums; a wave's loads of one row are 1 KiB contiguous, 16 rows
// in flight).  Of each row it keeps the 11 mask of its 64 individuals in two dwords: H & L of the lower 32 on the even bits, of the upper 32 on the odd bits.
// Then, 16 individuals at a time in ascending order, it loads their C weights into registers once and adds them to the accumulators of all kScoreRows rows
// under the mask (the weight's bits ANDed with 0 or -1).
// Individuals at and beyond indiv carry the weight zero, whatever the padding fields hold.  Reduction: the wave's shuffles, then (w0 + w1) + (w2 + w3) through
// the LDS; the order depends on indiv alone.  Rows [r0, r0 + kScoreRows) of the chunk's nrows; E is indexed by row0 + the row, as M is.
constexpr int kScoreRows = 16, kScoreCols = 1;   // (two columns a pass need 256 VGPRs and more: one wave per SIMD)

__global__ void __launch_bounds__(256) k_assoc_weights(const uint8_t *__restrict__ rows, long bps, long indiv, long row0, long nrows, const double *__restrict__ W,
                                                        long ldw, double *__restrict__ E, long lde, long blk0) {
  constexpr int C = kScoreCols;
  __shared__ double red[4][kScoreRows * C];
  const long r0 = (blk0 + blockIdx.x) * kScoreRows;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long nwords = (bps + 15) / 16;
  double acc[kScoreRows][C];
#pragma unroll
  for (int r = 0; r < kScoreRows; r++)
#pragma unroll
    for (int c = 0; c < C; c++) acc[r][c] = 0.0;
  for (long w = threadIdx.x; w < nwords; w += 256) {
    unsigned p0[kScoreRows], p1[kScoreRows];      // individuals 0-15: even bits of p0, 16-31: even bits of p1, 32-47: odd bits of p0, 48-63: odd bits of p1
#pragma unroll
    for (int r = 0; r < kScoreRows; r++) {
      p0[r] = 0u;
      p1[r] = 0u;
      if (r0 + r < nrows) {
        const uint8_t *row = rows + (size_t)(r0 + r) * (size_t)bps;
        const AssocWord a = assoc_load_word(row, w, bps, (int)(reinterpret_cast<uintptr_t>(row) & 15));
        const unsigned long long lo = a.lo & (a.lo >> 1) & 0x5555555555555555ull, hi = a.hi & (a.hi >> 1) & 0x5555555555555555ull;
        const unsigned long long p = lo | (hi << 1);
        p0[r] = (unsigned)p;
        p1[r] = (unsigned)(p >> 32);
      }
    }
#pragma unroll 1
    for (int step = 0; step < 4; step++) {          // 16 individuals a step: p0's even bits, then (p0, p1) <- (p1, p0 >> 1)
      const long i0 = 64 * w + 16 * step, left = indiv - i0;
      double wv[16][C];
#pragma unroll
      for (int k = 0; k < 16; k++)
#pragma unroll
        for (int c = 0; c < C; c++) wv[k][c] = k < left ? W[(size_t)c * (size_t)ldw + (size_t)(i0 + k)] : 0.0;
#pragma unroll
      for (int k = 0; k < 16; k++)                  // the rows innermost: consecutive adds go to different accumulators, none waits for the one before it
#pragma unroll
        for (int r = 0; r < kScoreRows; r++) {
          const int m = -(int)((p0[r] >> (2 * k)) & 1u);
#pragma unroll
          for (int c = 0; c < C; c++) acc[r][c] += __hiloint2double(__double2hiint(wv[k][c]) & m, __double2loint(wv[k][c]) & m);
        }
#pragma unroll
      for (int r = 0; r < kScoreRows; r++) {
        const unsigned cur = p0[r];
        p0[r] = p1[r];
        p1[r] = cur >> 1;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < kScoreRows; r++)
#pragma unroll
    for (int c = 0; c < C; c++) {
      double v = acc[r][c];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
      if (lane == 0) red[wave][r * C + c] = v;
    }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < kScoreRows * C && r0 + t / C < nrows)
    E[(size_t)(t % C) * (size_t)lde + (size_t)(row0 + r0 + t / C)] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}

// ---- the score test's epilogue: one thread per (SNP, trait), every operation rounded once in the header's order.  Columns of D and M: c = R, n + c = Wt,
// 2 n + c kh + j = H
__global__ void __launch_bounds__(256) k_assoc_score_finish(long snps, int n, int kh, const int *__restrict__ nobs, const int *__restrict__ c1,
                                                             const int *__restrict__ c2, const double *__restrict__ D, const double *__restrict__ M,
                                                             const double *__restrict__ E, long ld, double *__restrict__ score, double *__restrict__ var,
                                                             double *__restrict__ zstat, long ldo, long blk0) {
  const long idx = (blk0 + blockIdx.x) * 256 + threadIdx.x;
  if (idx >= snps * (long)n) return;
  const long s = idx % snps;
  const int c = (int)(idx / snps);
  const long N = nobs[s], Sz = (long)c1[s] + 2 * (long)c2[s];
  const double mu = __ddiv_rn((double)Sz, (double)N);
  const size_t ar = (size_t)s + (size_t)c * (size_t)ld, aw = (size_t)s + (size_t)(n + c) * (size_t)ld;
  const double U = __fma_rn(mu, M[ar], D[ar]);
  const double s2 = __fma_rn(2.0, E[ar], D[aw]);
  const double m2 = __dmul_rn(mu, mu);
  double sxx = __fma_rn(m2, M[aw], s2);
  for (int j = 0; j < kh; j++) {
    const size_t ah = (size_t)s + ((size_t)2 * (size_t)n + (size_t)c * (size_t)kh + (size_t)j) * (size_t)ld;
    const double a = __fma_rn(mu, M[ah], D[ah]);
    sxx = __fma_rn(-a, a, sxx);
  }
  const size_t o = (size_t)s + (size_t)c * (size_t)ldo;
  if (score) score[o] = U;
  if (var) var[o] = sxx;
  if (zstat) zstat[o] = __ddiv_rn(U, __dsqrt_rn(sxx));
}

// ---- host side
struct HandleHolder {                // the one-shot object is released on every exit path
  Handle *h = nullptr;
  ~HandleHolder() { if (h) destroy_handle(h); }
};
struct OneShotScope {                // this thread's products: single orientation, no warm-up, uncentred -- for the length of the call
  int single = tl_single_override, centered = tl_centered_override;
  bool no_warmup = tl_no_warmup;
  OneShotScope() { tl_single_override = 1; tl_no_warmup = true; tl_centered_override = 0; }
  ~OneShotScope() { tl_single_override = single; tl_no_warmup = no_warmup; tl_centered_override = centered; }
};

// rows of one staging chunk of a host matrix: MXA_ASSOC_CHUNK_ROWS, else what fits 256 MiB
long assoc_chunk_rows(long snps, long bps) {
  long rows = std::max<long>(1, (long)(((size_t)256 << 20) / (size_t)bps));
  const char *e = getenv("MXA_ASSOC_CHUNK_ROWS");
  if (e && atol(e) > 0) rows = atol(e);
  return std::min(rows, snps);
}

// *seen (host): a 01 field was met in an earlier pass; while it is clear the device flag is read once per call of this function, afterwards never again
int scan_rows(const uint8_t *d_rows, long bps, long indiv, long row0, long nrows, const AssocRow *d_bp, int ncols, int ncc, double *d_M, long snps, int *d_cnt,
              int *d_flag, bool *seen, hipStream_t s) {
  for (int cc = 0; cc < ncc; cc++) {
    if (cc == 1 && !*seen) {   // no missing call so far: M is zero (it was cleared) and the further column chunks need no pass
      int flag = 0;
      MXA_HIP(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
      MXA_HIP(hipStreamSynchronize(s));
      if (!flag) break;
      *seen = true;
    }
    launch_in_block_chunks(nrows, [&](unsigned nb, long b0) {
      k_assoc_scan<<<nb, 256, 0, s>>>(d_rows, bps, indiv, row0, d_bp + (size_t)cc * (size_t)indiv, cc * kAssocCols, ncols, d_M, snps, d_cnt, d_cnt + snps,
                                      d_cnt + 2 * snps, cc == 0, d_flag, b0);
    });
    MXA_HIP(hipGetLastError());
  }
  return 0;
}

// ---- what mxa_assoc_linear and mxa_assoc_score share: the device and the memory pre-flight, the one-shot object and the buffers of B (ncols columns), its
// row-packed copy, D, M, the counts and the device copies of host results (n columns each); the scan and the staging chunk by chunk; the product; the way out
struct AssocDriver {
  const char *who;
  long snps, indiv;
  int ncols, n;
  bool out_dev;
  int dev = -1, ncc = 0, max_n = 0;
  long bps = 0, chunk_rows = 0;
  bool in_place = false;
  size_t b_bytes = 0, bp_bytes = 0, dm_bytes = 0, cnt_bytes = 0, out_bytes = 0, bounce_bytes = 0;
  OneShotScope scope;
  HandleHolder obj;
  XBuf bB, bBp, bD, bM, bCnt, bFlag, bounce, bOut[3];
  Handle *h = nullptr;
  hipStream_t s = nullptr;
  double *out_d[3] = {nullptr, nullptr, nullptr};
  double *dB = nullptr, *dD = nullptr, *dM = nullptr;
  int *dCnt = nullptr, *dFlag = nullptr;
  AssocRow *dBp = nullptr;

  AssocDriver(const char *who_, long snps_, long indiv_, int ncols_, int n_, bool out_dev_) : who(who_), snps(snps_), indiv(indiv_), ncols(ncols_), n(n_), out_dev(out_dev_) {}

  // res: the caller's three results (nullable each); extra_bytes: device memory the caller allocates on top
  int begin(const unsigned char *plink, double *const res[3], size_t extra_bytes) {
    dev = select_device();
    if (dev < 0) return 1;
    ncc = (ncols + kAssocCols - 1) / kAssocCols;
    max_n = std::min(ncols, 32);
    bps = (indiv + 3) / 4;
    in_place = assoc_rows_in_place(plink, dev);   // rows in this device's memory are scanned where they lie
    chunk_rows = in_place ? snps : assoc_chunk_rows(snps, bps);
    // ---- memory pre-flight: the packed object, the staging chunk, B and its row-packed copy, D and M, the counts, the device copies of host results
    b_bytes = sizeof(double) * (size_t)indiv * (size_t)ncols;
    bp_bytes = sizeof(AssocRow) * (size_t)indiv * (size_t)ncc;
    dm_bytes = sizeof(double) * (size_t)snps * (size_t)ncols;
    cnt_bytes = sizeof(int) * 3 * (size_t)snps;
    out_bytes = sizeof(double) * (size_t)snps * (size_t)n;
    bounce_bytes = in_place ? 0 : (size_t)chunk_rows * (size_t)bps;
    const int n_out = (res[0] != nullptr) + (res[1] != nullptr) + (res[2] != nullptr);
    const size_t need = object_footprint(snps, indiv, max_n, true) + bounce_bytes + b_bytes + bp_bytes + 2 * dm_bytes + cnt_bytes + (out_dev ? 0 : n_out * out_bytes) + extra_bytes;
    size_t free_b = 0, total_b = 0;
    MXA_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b) { set_error(12, "%s: not enough device memory: required %zu MB, free %zu MB", who, need >> 20, free_b >> 20); return 1; }
    { void *o = nullptr; if (begin_handle(snps, indiv, max_n, &o, dev)) return 1; obj.h = reinterpret_cast<Handle *>(o); }
    h = obj.h;
    s = h->stream;
    if (bB.alloc(b_bytes) || bBp.alloc(bp_bytes) || bD.alloc(dm_bytes) || bM.alloc(dm_bytes) || bCnt.alloc(cnt_bytes) || bFlag.alloc(sizeof(int)) ||
        (!in_place && bounce.alloc(bounce_bytes))) return 1;
    for (int j = 0; j < 3; j++) {
      out_d[j] = res[j];
      if (!out_dev && res[j]) { if (bOut[j].alloc(out_bytes)) return 1; out_d[j] = (double *)bOut[j].p; }
    }
    dB = (double *)bB.p; dD = (double *)bD.p; dM = (double *)bM.p;
    dCnt = (int *)bCnt.p; dFlag = (int *)bFlag.p;
    dBp = (AssocRow *)bBp.p;
    return 0;
  }

  // the row-packed copy of the finished B; M and the flag cleared
  int pack_and_clear() {
    k_assoc_pack<<<dim3((unsigned)((indiv + 255) / 256), ncc), 256, 0, s>>>(dB, indiv, ncols, indiv, dBp);
    MXA_HIP(hipGetLastError());
    MXA_HIP(hipMemsetAsync(dM, 0, dm_bytes, s));
    MXA_HIP(hipMemsetAsync(dFlag, 0, sizeof(int), s));
    return 0;
  }

  // ---- the scan and the staging of the product operand, chunk by chunk, then D = Z^T B.  The uncentred product needs no allele frequencies: the object is
  // one without them (has_f cleared), which spares append_rows its own pass over the raw rows and makes a product that ignored tl_centered_override an error,
  // not a result.  per_chunk(d_rows, r0, nr): the caller's own pass over the chunk's raw rows on the device (0, or 1 with the error set).
  template <typename PerChunk>
  int scan_and_multiply(const unsigned char *plink, PerChunk &&per_chunk) {
    h->has_f = false;
    bool seen_missing = false;
    for (long r0 = 0; r0 < snps; r0 += chunk_rows) {
      const long nr = std::min(chunk_rows, snps - r0);
      const uint8_t *d_rows = plink + (size_t)r0 * (size_t)bps;
      if (!in_place) {
        MXA_HIP(hipMemcpyAsync(bounce.p, d_rows, (size_t)nr * (size_t)bps, hipMemcpyDefault, s));
        d_rows = (const uint8_t *)bounce.p;
      }
      if (scan_rows(d_rows, bps, indiv, r0, nr, dBp, ncols, ncc, dM, snps, dCnt, dFlag, &seen_missing, s)) return 1;
      if (per_chunk(d_rows, r0, nr)) return 1;
      if (append_rows(h, d_rows, r0, nr, nullptr)) return 1;
    }
    if (end_handle(h)) return 1;
    // in column chunks no wider than the object's max_n
    for (int c0 = 0; c0 < ncols; c0 += max_n) {
      const int w = std::min(max_n, ncols - c0);
      if (gemm_any(h, true, w, dB + (size_t)c0 * (size_t)indiv, indiv, dD + (size_t)c0 * (size_t)snps, snps, snps, false, false)) return 1;
    }
    return 0;
  }

  // host results and nobs, then the end of the stream
  int copy_out(double *const res[3], long ldo, int *nobs) {
    if (!out_dev) {
      const size_t ocol = sizeof(double) * (size_t)snps;
      for (int j = 0; j < 3; j++)
        if (res[j]) MXA_HIP(hipMemcpy2DAsync(res[j], sizeof(double) * (size_t)ldo, out_d[j], ocol, ocol, (size_t)n, hipMemcpyDeviceToHost, s));
    }
    if (nobs) MXA_HIP(hipMemcpyAsync(nobs, dCnt, sizeof(int) * (size_t)snps, hipMemcpyDefault, s));
    MXA_HIP(hipStreamSynchronize(s));
    return 0;
  }
};

int assoc_linear(const unsigned char *plink, long snps, long indiv, const double *Y, long ldy, int n, const double *Q, long ldq, int k, double *beta, double *se,
                 double *tstat, long ldo, int *nobs, int *dof, bool out_dev) {
  AssocDriver d("mxa_assoc_linear", snps, indiv, n + k, n, out_dev);
  double *const res[3] = {beta, se, tstat};
  if (d.begin(plink, res, 0)) return 1;
  const int ncols = n + k;
  hipStream_t s = d.s;
  XBuf bSmall;
  const size_t small_doubles = (size_t)ncols + (size_t)n + (size_t)n + (size_t)k * (size_t)n;   // T, syy, column sums, a = Q^T y
  if (bSmall.alloc(sizeof(double) * small_doubles)) return 1;
  double *dB = d.dB;
  double *dT = (double *)bSmall.p, *dSyy = dT + ncols, *dSum = dSyy + n, *dA = dSum + n;

  // ---- B = [Y~ | Q] on the device
  const size_t col = sizeof(double) * (size_t)indiv;
  MXA_HIP(hipMemcpy2DAsync(dB, col, Y, sizeof(double) * (size_t)ldy, col, (size_t)n, hipMemcpyDefault, s));
  double *dQ = dB + (size_t)n * (size_t)indiv;
  if (k > 0) MXA_HIP(hipMemcpy2DAsync(dQ, col, Q, sizeof(double) * (size_t)ldq, col, (size_t)k, hipMemcpyDefault, s));
  const unsigned iblocks = (unsigned)((indiv + 255) / 256);
  k_assoc_dots<<<dim3(1, n), 256, 0, s>>>(nullptr, 0, dB, indiv, indiv, dSum, 1, 0);
  k_assoc_center<<<dim3(iblocks, n), 256, 0, s>>>(dB, indiv, indiv, dSum);
  for (int pass = 0; pass < 2 && k > 0; pass++) {
    k_assoc_dots<<<dim3(k, n), 256, 0, s>>>(dQ, indiv, dB, indiv, indiv, dA, k, 0);
    k_assoc_project<<<dim3(iblocks, n), 256, 0, s>>>(dB, indiv, indiv, dQ, indiv, k, dA);
  }
  k_assoc_dots<<<dim3(1, n), 256, 0, s>>>(dB, indiv, dB, indiv, indiv, dSyy, 1, 1);
  k_assoc_dots<<<dim3(1, ncols), 256, 0, s>>>(nullptr, 0, dB, indiv, indiv, dT, 1, 0);
  if (d.pack_and_clear()) return 1;
  if (d.scan_and_multiply(plink, [](const uint8_t *, long, long) { return 0; })) return 1;

  const long total = snps * (long)n;
  launch_in_block_chunks((total + 255) / 256, [&](unsigned nb, long b0) {
    k_assoc_finish<<<nb, 256, 0, s>>>(snps, n, k, d.dCnt, d.dCnt + snps, d.dCnt + 2 * snps, d.dD, d.dM, snps, dT, dSyy, (double)(indiv - k - 2), d.out_d[0], d.out_d[1],
                                      d.out_d[2], out_dev ? ldo : snps, b0);
  });
  MXA_HIP(hipGetLastError());
  if (d.copy_out(res, ldo, nobs)) return 1;
  if (dof) *dof = (int)(indiv - k - 2);
  return 0;
}

// B = [R | Wt | H]: column c of R, column n + c of Wt, columns 2 n + c kh + j of H belong to trait c.  after: a stage of another unit follows the epilogue
// (mxa_assoc_stage.h)
int assoc_score(const unsigned char *plink, long snps, long indiv, const double *R, long ldr, const double *Wt, long ldw, const double *H, long ldh, int n, int kh,
                double *score, double *var, double *zstat, long ldo, int *nobs, bool out_dev, const AssocAfterScan *after = nullptr) {
  const int ncols = n * (kh + 2);
  AssocDriver d(after ? after->who : "mxa_assoc_score", snps, indiv, ncols, n, out_dev);
  double *const res[3] = {score, var, zstat};
  const size_t e_bytes = sizeof(double) * (size_t)snps * (size_t)n;
  size_t extra = e_bytes;                       // E
  if (after) {                                  // the stage's own memory, and an array for every result it reads that the caller did not give
    extra += after->extra_bytes;
    for (int j = 0; j < 3; j++)
      if (after->reads[j] && !res[j]) extra += e_bytes;
  }
  if (d.begin(plink, res, extra)) return 1;
  hipStream_t s = d.s;
  XBuf bE, bOwn[3];
  if (bE.alloc(e_bytes)) return 1;
  const long ldu = out_dev ? ldo : snps;
  for (int j = 0; j < 3 && after; j++)
    if (after->reads[j] && !d.out_d[j]) { if (bOwn[j].alloc(sizeof(double) * (size_t)ldu * (size_t)n)) return 1; d.out_d[j] = (double *)bOwn[j].p; }
  double *dE = (double *)bE.p;
  const size_t col = sizeof(double) * (size_t)indiv;
  double *dW = d.dB + (size_t)n * (size_t)indiv, *dH = d.dB + (size_t)2 * (size_t)n * (size_t)indiv;
  MXA_HIP(hipMemcpy2DAsync(d.dB, col, R, sizeof(double) * (size_t)ldr, col, (size_t)n, hipMemcpyDefault, s));
  MXA_HIP(hipMemcpy2DAsync(dW, col, Wt, sizeof(double) * (size_t)ldw, col, (size_t)n, hipMemcpyDefault, s));
  if (kh > 0)
    MXA_HIP(hipMemcpy2DAsync(dH, col, H, sizeof(double) * (size_t)ldh, col, (size_t)n * (size_t)kh, hipMemcpyDefault, s));
  if (d.pack_and_clear()) return 1;
  const long bps = d.bps;
  auto weights = [&](const uint8_t *d_rows, long r0, long nr) -> int {          // E: kScoreCols weight columns a pass
    for (int c0 = 0; c0 < n; c0 += kScoreCols) {
      const double *w = dW + (size_t)c0 * (size_t)indiv;
      double *e = dE + (size_t)c0 * (size_t)snps;
      launch_in_block_chunks((nr + kScoreRows - 1) / kScoreRows, [&](unsigned nb, long b0) {
        k_assoc_weights<<<nb, 256, 0, s>>>(d_rows, bps, indiv, r0, nr, w, indiv, e, snps, b0);
      });
      MXA_HIP(hipGetLastError());
    }
    return 0;
  };
  if (d.scan_and_multiply(plink, weights)) return 1;
  const long total = snps * (long)n;
  launch_in_block_chunks((total + 255) / 256, [&](unsigned nb, long b0) {
    k_assoc_score_finish<<<nb, 256, 0, s>>>(snps, n, kh, d.dCnt, d.dCnt + snps, d.dCnt + 2 * snps, d.dD, d.dM, dE, snps, d.out_d[0], d.out_d[1], d.out_d[2],
                                            ldu, b0);
  });
  MXA_HIP(hipGetLastError());
  if (after) {
    const AssocScanView v = {snps, indiv, bps, n, kh, d.in_place, out_dev, s, d.dCnt, d.dCnt + snps, d.dCnt + 2 * snps, d.dD, d.dM, dW, dH,
                             d.out_d[0], d.out_d[1], d.out_d[2], ldu};
    if (after->run(after->self, v, plink)) return 1;
  }
  return d.copy_out(res, ldo, nobs);
}

}  // namespace

int assoc_score_then(const unsigned char *plink, long snps, long indiv, const double *R, long ldr, const double *Wt, long ldw, const double *H, long ldh, int n, int kh,
                     double *score, double *var, double *zstat, long ldo, int *nobs, bool out_dev, const AssocAfterScan &after) {
  return assoc_score(plink, snps, indiv, R, ldr, Wt, ldw, H, ldh, n, kh, score, var, zstat, ldo, nobs, out_dev, &after);
}

}  // namespace mxa

extern "C" int mxa_assoc_basis(int indiv, const double *W, long ldw, int q, double *Q, long ldq) {
  using namespace mxa;
  clear_error();
  const char *who = "mxa_assoc_basis";
  if (indiv < 1 || q < 0) { set_error(1, "%s: indiv must be positive and q must not be negative", who); return 1; }
  if (!W || !Q) { set_error(1, "%s: W and Q must not be NULL", who); return 1; }
  if (ldw < indiv || ldq < indiv) { set_error(1, "%s: need ldw >= indiv and ldq >= indiv (ldw %ld, ldq %ld, indiv %d)", who, ldw, ldq, indiv); return 1; }
  if (q == 0) return 0;
  int bad = -1;
  const int rc = assoc_basis_host(indiv, W, ldw, q, Q, ldq, &bad);
  if (rc == 2) { set_error(1, "%s: column %d of W holds a non-finite entry", who, bad); return 1; }
  if (rc == 3) { set_error(1, "%s: column %d of W is constant or depends on the columns before it", who, bad); return 1; }
  return 0;
}

extern "C" int mxa_assoc_linear(const unsigned char *plink, int snps, int indiv, const double *Y, long ldy, int n, const double *Q, long ldq, int k, double *beta,
                                double *se, double *tstat, long ldo, int *nobs, int *dof) {
  using namespace mxa;
  clear_error();
  const char *who = "mxa_assoc_linear";
  const char *bad = assoc_linear_args(plink, snps, indiv, Y, ldy, n, Q, ldq, k, beta, se, tstat, ldo);
  if (bad) { set_error(1, "%s: %s", who, bad); return 1; }
  bool out_dev = false;
  if (results_on_one_side(who, "beta, se and tstat", {beta, se, tstat}, &out_dev)) return 1;
  DeviceRestore restore;
  return assoc_linear(plink, snps, indiv, Y, ldy, n, Q, ldq, k, beta, se, tstat, ldo, nobs, dof, out_dev);
}

extern "C" int mxa_assoc_logistic_null(int indiv, const double *y, const double *W, long ldw, int q, double tol, int max_iter, double *gamma, double *r, double *w,
                                       double *H, long ldh, int *iters) {
  using namespace mxa;
  clear_error();
  const char *who = "mxa_assoc_logistic_null";
  const char *wrong = assoc_logistic_null_args(indiv, y, W, ldw, q, gamma, r, w, H, ldh);
  if (wrong) { set_error(1, "%s: %s", who, wrong); return 1; }
  long bad = -1;
  int rc = 0;
  try {
    rc = assoc_logistic_null_host(indiv, y, W, ldw, q, tol, max_iter, gamma, r, w, H, ldh, iters, &bad);
  } catch (const std::bad_alloc &) {          // the work arrays (2 indiv long doubles) come before the first output is written
    set_error(12, "%s: not enough host memory for the work arrays of %d individuals", who, indiv);
    return 1;
  }
  if (rc == 2) { set_error(1, "%s: column %ld of W holds a non-finite entry", who, bad); return 1; }
  if (rc == 3) { set_error(1, "%s: y[%ld] is not exactly 0 or 1", who, bad); return 1; }
  if (rc == 4) { set_error(1, "%s: all entries of y are equal", who); return 1; }
  if (rc == 5) {
    if (bad == 0) set_error(1, "%s: C^T diag(w) C is not positive definite at the intercept", who);
    else set_error(1, "%s: C^T diag(w) C is not positive definite: column %ld of W is constant or depends on the columns before it", who, bad - 1);
    return 1;
  }
  if (rc == 6) { set_error(1, "%s: no convergence within %d iterations (separation?)", who, max_iter); return 1; }
  return 0;
}

extern "C" int mxa_assoc_score(const unsigned char *plink, int snps, int indiv, const double *R, long ldr, const double *Wt, long ldw, const double *H, long ldh, int n,
                               int kh, double *score, double *var, double *zstat, long ldo, int *nobs) {
  using namespace mxa;
  clear_error();
  const char *who = "mxa_assoc_score";
  const char *bad = assoc_score_args(plink, snps, indiv, R, ldr, Wt, ldw, H, ldh, n, kh, score, var, zstat, ldo);
  if (bad) { set_error(1, "%s: %s", who, bad); return 1; }
  bool out_dev = false;
  if (results_on_one_side(who, "score, var and zstat", {score, var, zstat}, &out_dev)) return 1;
  DeviceRestore restore;
  return assoc_score(plink, snps, indiv, R, ldr, Wt, ldw, H, ldh, n, kh, score, var, zstat, ldo, nobs, out_dev);
}

