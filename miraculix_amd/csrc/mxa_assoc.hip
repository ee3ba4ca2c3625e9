// mxa_assoc.hip -- the association scan: per-SNP linear regression y_c ~ 1 + Q + x_s on packed genotypes (include/miraculix_amd.h: mxa_assoc_linear; DESIGN.md
// 3.6e).  The fp64 product does the work: D = Z^T B for B = [Y~ | Q] is the library's own uncentred 'T' product on a one-shot object.  What the product cannot
// know -- the missing calls -- comes from ONE streaming pass over the raw PLINK rows (k_assoc_scan): the exact counts N, c1, c2 of every SNP by popcount, and
// M_b = the sum of b over the SNP's missing individuals.  k_assoc_finish turns D, M and the counts into beta, se and t in the documented operation order.
// The score test for binary traits (mxa_assoc_score) is the same scan with B = [R | Wt | H] and one more sum per weight column, E = the weights
// summed over the SNP's 11 fields (k_assoc_weights, dense); k_assoc_score_finish is its epilogue.  Its null model is host code: mxa_assoc_null_host.h.
// mxa_assoc_score_spa is that scan followed by the saddlepoint correction of the SNPs with |z| >= z_cutoff: the k_assoc_spa* kernels.
// mxa_assoc_score_firth is the same scan and the same stage with another solve: the (Firth-penalised) fit of the SNP's effect, k_assoc_firth*.
// mxa_assoc_set is the same scan followed by the stage of another unit, mxa_assoc_set.hip, through assoc_score_then (mxa_assoc_stage.h).
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

// ---- the sums of the phenotype preparation: 256 threads, thread t takes the individuals t, t + 256, ... in ascending order, then a fixed tree -- the wave's
// shuffles (32, 16, ..., 1), then (w0 + w1) + (w2 + w3) through the LDS.  The order depends on indiv alone.
__device__ __forceinline__ double assoc_block_sum(double v, double *red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave] = v;
  __syncthreads();
  const double r = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return r;
}

// out[x + y ld_out] = sum_i A[i, a] B[i, y] with a = x (diag == 0) or a = y (diag != 0: the squared norms, launched with gridDim.x == 1); A == nullptr: the
// column sums of B.  One workgroup per output.
__global__ void __launch_bounds__(256) k_assoc_dots(const double *__restrict__ A, long lda, const double *__restrict__ B, long ldb, long indiv,
                                                     double *__restrict__ out, int ld_out, int diag) {
  __shared__ double red[4];
  const double *b = B + (size_t)blockIdx.y * (size_t)ldb;
  const double *a = A ? A + (size_t)(diag ? blockIdx.y : blockIdx.x) * (size_t)lda : nullptr;
  double acc = 0.0;
  for (long i = threadIdx.x; i < indiv; i += 256) acc = a ? __fma_rn(a[i], b[i], acc) : acc + b[i];
  const double s = assoc_block_sum(acc, red);
  if (threadIdx.x == 0) out[(size_t)blockIdx.x + (size_t)blockIdx.y * (size_t)ld_out] = s;
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

// ---- the saddlepoint correction of the score test (mxa_assoc_score_spa).  After k_assoc_score_finish: k_assoc_spa_classify writes the normal
// p-value and the flag 0 / 3 of every (SNP, trait) and marks with 1 what is to be corrected; k_assoc_spa_list compacts the marked SNPs in ascending order (one
// workgroup, prefix sums: no atomics, so the list is the same in every run) and k_assoc_spa_items names their (SNP, trait) items.  Then per batch of marked
// SNPs: k_assoc_spa_form writes the adjusted genotype g of every item, k_assoc_spa solves both sides of every item, k_assoc_spa_combine writes p and the flag.
constexpr int kSpaTile = 8;                                     // marked SNPs one workgroup of k_assoc_spa_form decodes for its 256 individuals
constexpr int kSpaOutside = 0, kSpaFailed = 1, kSpaSolved = 2;  // what a side ends as
struct SpaSide { double tail; int status; int evals; };

// tau_{c,j,i} = h_{c,j,i} / w_{c,i}, once per call; blockIdx.y = c kh + j
__global__ void __launch_bounds__(256) k_assoc_spa_tau(const double *__restrict__ H, const double *__restrict__ W, long indiv, int kh, double *__restrict__ Ht) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= indiv) return;
  const size_t at = (size_t)blockIdx.y * (size_t)indiv + (size_t)i;
  Ht[at] = __ddiv_rn(H[at], W[(size_t)(blockIdx.y / (unsigned)kh) * (size_t)indiv + (size_t)i]);
}

// one thread per (SNP, trait): flag 3 and NaN where z is not finite, else the normal p-value erfc(|z| sqrt(1/2)) and the flag 0, or the mark 1 where |z| >=
// z_cutoff (the normal p-value stays where the correction ends with the flag 2).  pval and flag: snps x n, ld snps.
__global__ void __launch_bounds__(256) k_assoc_spa_classify(long snps, int n, const double *__restrict__ zstat, long ldz, double z_cutoff, double *__restrict__ pval,
                                                             int *__restrict__ flag, long blk0) {
  const long idx = (blk0 + blockIdx.x) * 256 + threadIdx.x;
  if (idx >= snps * (long)n) return;
  const long s = idx % snps;
  const double z = zstat[(size_t)s + (size_t)(idx / snps) * (size_t)ldz];
  if (!isfinite(z)) { flag[idx] = 3; pval[idx] = __longlong_as_double(0x7ff8000000000000ll); return; }
  const double az = fabs(z);
  flag[idx] = az < z_cutoff ? 0 : 1;
  pval[idx] = erfc(__dmul_rn(az, 0.70710678118654752440));
}

// exclusive prefix sum over the workgroup's 256 threads through the LDS; *total = the sum of all
__device__ __forceinline__ long spa_block_scan(long v, long *sh, long *total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const long add = t >= off ? sh[t - off] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  const long incl = sh[t];
  *total = sh[255];
  __syncthreads();
  return incl - v;
}

// ONE workgroup: list[k] = the k-th SNP with a marked trait, ascending; off[k] = the index of its first item (its marked traits, ascending, follow one
// another); off[count[0]] = count[1] = the number of items, count[0] = the number of marked SNPs
__global__ void __launch_bounds__(256) k_assoc_spa_list(long snps, int n, const int *__restrict__ flag, int *__restrict__ list, long *__restrict__ off,
                                                         long *__restrict__ count) {
  __shared__ long sh[256];
  long base_k = 0, base_item = 0;
  for (long s0 = 0; s0 < snps; s0 += 256) {
    const long s = s0 + threadIdx.x;
    long cnt = 0;
    if (s < snps)
      for (int c = 0; c < n; c++) cnt += flag[(size_t)s + (size_t)c * (size_t)snps] == 1;
    long tot_k = 0, tot_item = 0;
    const long k = base_k + spa_block_scan(cnt > 0, sh, &tot_k);
    const long item = base_item + spa_block_scan(cnt, sh, &tot_item);
    if (cnt > 0) { list[k] = (int)s; off[k] = item; }
    base_k += tot_k;
    base_item += tot_item;
  }
  if (threadIdx.x == 0) { off[base_k] = base_item; count[0] = base_k; count[1] = base_item; }
}

// one thread per marked SNP: the SNP and the trait of each of its items
__global__ void __launch_bounds__(256) k_assoc_spa_items(long nk, long snps, int n, const int *__restrict__ flag, const int *__restrict__ list, const long *__restrict__ off,
                                                          int *__restrict__ item_s, int *__restrict__ item_c, long blk0) {
  const long k = (blk0 + blockIdx.x) * 256 + threadIdx.x;
  if (k >= nk) return;
  const long s = list[k];
  long at = off[k];
  for (int c = 0; c < n; c++)
    if (flag[(size_t)s + (size_t)c * (size_t)snps] == 1) { item_s[at] = (int)s; item_c[at] = c; at++; }
}

// (a) g of the items of the marked SNPs [k0, k1): workgroup (tile, ib) = divmod(blk0 + blockIdx.x, iblocks) takes the individuals 256 ib + t of the kSpaTile
// marked SNPs from k0 + kSpaTile tile on.  Every thread decodes its field of each of these rows once (00 -> 0, 01 -> mu, 10 -> 1, 11 -> 2; mu = Sz / N as in
// k_assoc_score_finish), then per trait c with an item in the tile reads tau_{c,j,i} once per j and applies it to all of the tile's SNPs with that item:
// g = x, then g = fma(-a_j, tau_j, g) over ascending j with a_j = fma(mu, M_hj, D_hj) (the workgroup's own loads of M and D are uniform).  rows: the raw
// matrix (compact == 0: row list[k]) or the bounce buffer of the batch (compact != 0: row k - k0).  G: item off[k0] is its first row of indiv doubles.
__global__ void __launch_bounds__(256) k_assoc_spa_form(const uint8_t *__restrict__ rows, long bps, int compact, long indiv, long snps, int n, int kh,
                                                         const int *__restrict__ list, const long *__restrict__ off, long k0, long k1, const int *__restrict__ flag,
                                                         const int *__restrict__ nobs, const int *__restrict__ c1, const int *__restrict__ c2,
                                                         const double *__restrict__ D, const double *__restrict__ M, const double *__restrict__ Ht,
                                                         double *__restrict__ G, long iblocks, long blk0) {
  const long b = blk0 + blockIdx.x;
  const long kt = k0 + (b / iblocks) * kSpaTile;
  const long i = (b % iblocks) * 256 + threadIdx.x;
  const bool live = i < indiv;
  const long item_base = off[k0];
  double x[kSpaTile], mu[kSpaTile];
  long s[kSpaTile], item[kSpaTile];
#pragma unroll
  for (int u = 0; u < kSpaTile; u++) {
    x[u] = 0.0; mu[u] = 0.0; s[u] = -1; item[u] = 0;
    const long k = kt + u;
    if (k < k1) {
      s[u] = list[k];
      item[u] = off[k] - item_base;
      mu[u] = __ddiv_rn((double)((long)c1[s[u]] + 2 * (long)c2[s[u]]), (double)nobs[s[u]]);
      if (live) {
        const uint8_t *row = rows + (size_t)(compact ? k - k0 : s[u]) * (size_t)bps;
        const int code = (row[i >> 2] >> (2 * (int)(i & 3))) & 3;
        x[u] = code == 0 ? 0.0 : code == 1 ? mu[u] : code == 2 ? 1.0 : 2.0;
      }
    }
  }
  for (int c = 0; c < n; c++) {
    bool on[kSpaTile];
    bool any = false;
#pragma unroll
    for (int u = 0; u < kSpaTile; u++) { on[u] = s[u] >= 0 && flag[(size_t)s[u] + (size_t)c * (size_t)snps] == 1; any = any || on[u]; }
    if (!any) continue;
    double g[kSpaTile];
#pragma unroll
    for (int u = 0; u < kSpaTile; u++) g[u] = x[u];
    for (int j = 0; j < kh; j++) {
      const size_t col = (size_t)c * (size_t)kh + (size_t)j;
      const double tau = live ? Ht[col * (size_t)indiv + (size_t)i] : 0.0;
#pragma unroll
      for (int u = 0; u < kSpaTile; u++)
        if (on[u]) {
          const size_t ah = (size_t)s[u] + ((size_t)2 * (size_t)n + col) * (size_t)snps;
          const double a = __fma_rn(mu[u], M[ah], D[ah]);
          g[u] = __fma_rn(-a, tau, g[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < kSpaTile; u++)
      if (on[u]) {
        if (live) G[(size_t)item[u] * (size_t)indiv + (size_t)i] = g[u];
        item[u]++;
      }
  }
}

// K sums of a workgroup at once, in the order of assoc_block_sum: every thread returns with the K totals
template <int K>
__device__ __forceinline__ void spa_block_sums(double (&v)[K], double (*red)[4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < K; q++) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v[q] += __shfl_down(v[q], off, 64);
    if (lane == 0) red[q][wave] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < K; q++) v[q] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
  __syncthreads();
}

// (b) one workgroup per (item, side): item = blk0 + blockIdx.x >> 1 of the batch (row `item` of G), side 0: sigma = +1, side 1: sigma = -1.  Thread t takes the
// individuals t, t + 256, ... in ascending order; every sum ends in spa_block_sums, so its order depends on indiv alone.  First c0, A, G+ and G-, then Newton
// from t = 0 with its bracket, entirely in the kernel: an evaluation reads g and p once and sums K' and K'' (the accepted t^: K and K''), thread 0 updates t,
// the bracket and the state and broadcasts both through the LDS.  The header of mxa_assoc_score_spa has the rules.
__global__ void __launch_bounds__(256) k_assoc_spa(const double *__restrict__ G, long indiv, const double *__restrict__ P, const int *__restrict__ item_s,
                                                    const int *__restrict__ item_c, long item_base, long nitems, const double *__restrict__ score, long ldu, double tol,
                                                    int max_iter, SpaSide *__restrict__ out, long blk0) {
  __shared__ double red[4][4];
  __shared__ double sh_t;
  __shared__ int sh_state;                      // 0: a Newton evaluation is next, 1: the evaluation at the accepted t^ is next, 2: done
  const long w = blk0 + blockIdx.x;
  const long item = w >> 1;
  if (item >= nitems) return;
  const double sigma = (w & 1) ? -1.0 : 1.0;
  const double *g = G + (size_t)item * (size_t)indiv;
  const long s = item_s[item_base + item];
  const int c = item_c[item_base + item];
  const double *p = P + (size_t)c * (size_t)indiv;
  double v4[4] = {0.0, 0.0, 0.0, 0.0};
  for (long i = threadIdx.x; i < indiv; i += 256) {
    const double gi = g[i];
    v4[0] = __fma_rn(gi, p[i], v4[0]);
    v4[1] += fabs(gi);
    v4[2] += fmax(gi, 0.0);
    v4[3] += fmin(gi, 0.0);
  }
  spa_block_sums<4>(v4, red);
  const double c0 = v4[0], A = v4[1];
  const double q = sigma * fabs(score[(size_t)s + (size_t)c * (size_t)ldu]);
  const double margin = sigma * (((w & 1) ? v4[3] : v4[2]) - c0 - q);
  if (threadIdx.x == 0) {
    sh_t = 0.0;
    sh_state = 0;
    if (margin <= 0x1p-30 * A) { out[w].tail = 0.0; out[w].status = kSpaOutside; out[w].evals = 0; sh_state = 2; }
  }
  __syncthreads();
  int state = __builtin_amdgcn_readfirstlane(sh_state);
  double t = sh_t, lo = -INFINITY, hi = INFINITY;
  int evals = 0;
  while (state != 2) {
    double v3[3] = {0.0, 0.0, 0.0};            // K (state 1 only), K' (state 0 only), K''
    for (long i = threadIdx.x; i < indiv; i += 256) {
      const double gi = g[i], pi = p[i];
      const double x = t * gi;
      const double e = exp(-fabs(x));
      const bool pos = x >= 0.0;
      const double al = pos ? pi : 1.0 - pi, be = pos ? 1.0 - pi : pi;
      const double d = al + be * e, r = 1.0 / d;  // one division a term: K' and K'' take the reciprocal
      if (state == 1) v3[0] += fmax(x, 0.0) + log(d);
      else v3[1] += gi * ((pos ? pi : pi * e) * r);
      v3[2] += (gi * r) * (gi * r) * (al * be * e);
    }
    spa_block_sums<3>(v3, red);
    if (threadIdx.x == 0) {
      int status = -1;                           // -1: go on
      double tail = 0.0;
      if (state == 1) {
        const double K = v3[0] - t * c0;
        const double r = sqrt(2.0 * (t * q - K));
        const double ws = t > 0.0 ? r : t < 0.0 ? -r : 0.0;
        const double vs = t * sqrt(v3[2]);
        const double zeta = ws + log(vs / ws) / ws;
        status = isfinite(zeta) ? kSpaSolved : kSpaFailed;
        if (status == kSpaSolved) tail = 0.5 * erfc(sigma * zeta * 0.70710678118654752440);
      } else {
        evals++;
        const double f = (v3[1] - c0) - q;
        if (f < 0.0) lo = t; else hi = t;
        double tn = t - f / v3[2];
        if (!isfinite(tn)) status = kSpaFailed;
        else if (fabs(tn - t) <= tol * fabs(tn)) { sh_t = tn; sh_state = 1; }
        else {
          if (!(tn > lo && tn < hi)) tn = 0.5 * (lo + hi);
          if (!isfinite(tn) || evals >= max_iter) status = kSpaFailed;
          else sh_t = tn;
        }
      }
      if (status >= 0) { out[w].tail = tail; out[w].status = status; out[w].evals = evals; sh_state = 2; }
    }
    __syncthreads();
    state = __builtin_amdgcn_readfirstlane(sh_state);
    t = sh_t;
  }
}

// one thread per item of the batch: the two sides combined.  The normal p-value that k_assoc_spa_classify left stays with the flag 2.
__global__ void __launch_bounds__(256) k_assoc_spa_combine(long nitems, long item_base, const int *__restrict__ item_s, const int *__restrict__ item_c,
                                                            const double *__restrict__ score, long ldu, const SpaSide *__restrict__ side, long snps,
                                                            double *__restrict__ pval, int *__restrict__ flag, long blk0) {
  const long item = (blk0 + blockIdx.x) * 256 + threadIdx.x;
  if (item >= nitems) return;
  const long s = item_s[item_base + item];
  const int c = item_c[item_base + item];
  const int obs = score[(size_t)s + (size_t)c * (size_t)ldu] >= 0.0 ? 0 : 1;
  const SpaSide a = side[2 * item + obs], b = side[2 * item + (1 - obs)];
  const size_t o = (size_t)s + (size_t)c * (size_t)snps;
  if (a.status != kSpaSolved || b.status == kSpaFailed) { flag[o] = 2; return; }
  flag[o] = 1;
  pval[o] = a.tail + (b.status == kSpaSolved ? b.tail : 0.0);
}

// ---- the effect sizes of the score test (mxa_assoc_score_firth): the stage of the saddlepoint correction with its own classify epilogue, solve
// and combine.  k_assoc_firth_classify writes the one-step values and the flag 0 / 3 of every (SNP, trait) and marks with 1 what is to be fitted (the one-step
// values stay where the fit ends with the flag 2); beta, se, chisq, pval and flag: snps x n, ld snps.
struct FirthFit { double beta, K, k2, k20; int status, evals; };   // beta^, K(beta^), K''(beta^), K''(0)

__global__ void __launch_bounds__(256) k_assoc_firth_classify(long snps, int n, const double *__restrict__ score, const double *__restrict__ var,
                                                               const double *__restrict__ zstat, long ldu, double z_cutoff, double *__restrict__ beta,
                                                               double *__restrict__ se, double *__restrict__ chisq, double *__restrict__ pval, int *__restrict__ flag,
                                                               long blk0) {
  const long idx = (blk0 + blockIdx.x) * 256 + threadIdx.x;
  if (idx >= snps * (long)n) return;
  const size_t at = (size_t)(idx % snps) + (size_t)(idx / snps) * (size_t)ldu;
  const double z = zstat[at];
  if (!isfinite(z)) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    flag[idx] = 3; beta[idx] = nan; se[idx] = nan; chisq[idx] = nan; pval[idx] = nan;
    return;
  }
  const double az = fabs(z), V = var[at];
  flag[idx] = az < z_cutoff ? 0 : 1;
  beta[idx] = __ddiv_rn(score[at], V);
  se[idx] = __ddiv_rn(1.0, __dsqrt_rn(V));
  chisq[idx] = __dmul_rn(z, z);
  pval[idx] = erfc(__dmul_rn(az, 0.70710678118654752440));
}

// one workgroup per item: row `item` = blk0 + blockIdx.x of G, one solve.  Thread t takes the individuals t, t + 256, ... in ascending order; every sum ends in
// spa_block_sums, so its order depends on indiv alone.  First c0, A, G+ and G- (penalty == 0: the support test of the observed side), then Newton from beta = 0
// with its bracket, entirely in the kernel: an evaluation reads g and p once and sums K1, K2 and, with the penalty, K3 and K4 (the derivatives of K) -- one exp
// and one division a term, the two further sums are FMA chains on g r and omega; the evaluation at the accepted beta^ sums K and K2.  Thread 0 updates beta, the
// bracket and the state and broadcasts both through the LDS.  penalty is uniform over the launch.  The header of mxa_assoc_score_firth has the rules.
__global__ void __launch_bounds__(256) k_assoc_firth(const double *__restrict__ G, long indiv, const double *__restrict__ P, const int *__restrict__ item_s,
                                                      const int *__restrict__ item_c, long item_base, long nitems, const double *__restrict__ score, long ldu,
                                                      int penalty, double tol, int max_iter, FirthFit *__restrict__ out, long blk0) {
  __shared__ double red[4][4];
  __shared__ double sh_b;
  __shared__ int sh_state;                      // 0: a Newton evaluation is next, 1: the evaluation at the accepted beta^ is next, 2: done
  const long item = blk0 + blockIdx.x;
  if (item >= nitems) return;
  const double *g = G + (size_t)item * (size_t)indiv;
  const long s = item_s[item_base + item];
  const int c = item_c[item_base + item];
  const double *p = P + (size_t)c * (size_t)indiv;
  double v4[4] = {0.0, 0.0, 0.0, 0.0};
  for (long i = threadIdx.x; i < indiv; i += 256) {
    const double gi = g[i];
    v4[0] = __fma_rn(gi, p[i], v4[0]);
    v4[1] += fabs(gi);
    v4[2] += fmax(gi, 0.0);
    v4[3] += fmin(gi, 0.0);
  }
  spa_block_sums<4>(v4, red);
  const double c0 = v4[0], A = v4[1];
  const double U = score[(size_t)s + (size_t)c * (size_t)ldu];
  if (threadIdx.x == 0) {
    sh_b = 0.0;
    sh_state = 0;
    const double margin = U >= 0.0 ? (v4[2] - c0) - U : -((v4[3] - c0) - U);
    if (penalty == 0 && margin <= 0x1p-30 * A) {   // the statistic lies on the edge of its support: the unpenalised likelihood has no maximum
      out[item].beta = 0.0; out[item].K = 0.0; out[item].k2 = 0.0; out[item].k20 = 0.0; out[item].status = kSpaOutside; out[item].evals = 0;
      sh_state = 2;
    }
  }
  __syncthreads();
  int state = __builtin_amdgcn_readfirstlane(sh_state);
  double b = sh_b, lo = -INFINITY, hi = INFINITY, k20 = 0.0;
  int evals = 0;
  while (state != 2) {
    double v2[2] = {0.0, 0.0}, w2[2] = {0.0, 0.0};   // K (state 1) or K1 (state 0), K2; K3, K4 (state 0 with the penalty)
    for (long i = threadIdx.x; i < indiv; i += 256) {
      const double gi = g[i], pi = p[i];
      const double x = b * gi;
      const double e = exp(-fabs(x));
      const bool pos = x >= 0.0;
      const double al = pos ? pi : 1.0 - pi, be = pos ? 1.0 - pi : pi;
      const double d = al + be * e, r = 1.0 / d;  // one division a term
      const double gr = gi * r, abe = al * be * e, t2 = gr * gr * abe;   // t2 = g^2 omega
      if (state == 1) v2[0] += fmax(x, 0.0) + log(d);
      else {
        const double pr = (pos ? pi : pi * e) * r;
        v2[0] += gi * pr;
        if (penalty) {
          const double t3 = t2 * gi;
          w2[0] = fma(t3, 1.0 - 2.0 * pr, w2[0]);
          w2[1] = fma(t3 * gi, 1.0 - 6.0 * (abe * r * r), w2[1]);
        }
      }
      v2[1] += t2;
    }
    spa_block_sums<2>(v2, red);
    if (penalty && state == 0) spa_block_sums<2>(w2, red);
    if (threadIdx.x == 0) {
      int status = -1;                           // -1: go on
      double K = 0.0;
      if (state == 1) {
        K = v2[0] - b * c0;
        status = kSpaSolved;
      } else {
        evals++;
        const double K2 = v2[1];
        if (evals == 1) k20 = K2;
        double f = (v2[0] - c0) - U, fp = K2;
        if (penalty) {
          const double r3 = w2[0] / K2;
          f -= 0.5 * r3;
          const double alt = K2 - 0.5 * (w2[1] / K2 - r3 * r3);
          if (alt > 0.0) fp = alt;
        }
        if (f < 0.0) lo = b; else hi = b;
        double bn = b - f / fp;
        if (!isfinite(bn)) status = kSpaFailed;
        else if (fabs(bn - b) <= tol * fabs(bn)) { sh_b = bn; sh_state = 1; }
        else {
          if (!(bn > lo && bn < hi)) bn = 0.5 * (lo + hi);
          if (!isfinite(bn) || evals >= max_iter) status = kSpaFailed;
          else sh_b = bn;
        }
      }
      if (status >= 0) {
        out[item].beta = b; out[item].K = K; out[item].k2 = v2[1]; out[item].k20 = k20; out[item].status = status; out[item].evals = evals;
        sh_state = 2;
      }
    }
    __syncthreads();
    state = __builtin_amdgcn_readfirstlane(sh_state);
    b = sh_b;
  }
}

// one thread per item of the batch: the results of a converged fit.  The one-step values that k_assoc_firth_classify left stay with the flag 2.
__global__ void __launch_bounds__(256) k_assoc_firth_combine(long nitems, long item_base, const int *__restrict__ item_s, const int *__restrict__ item_c,
                                                              const double *__restrict__ score, long ldu, const FirthFit *__restrict__ fit, int penalty, long snps,
                                                              double *__restrict__ beta, double *__restrict__ se, double *__restrict__ chisq,
                                                              double *__restrict__ pval, int *__restrict__ flag, long blk0) {
  const long item = (blk0 + blockIdx.x) * 256 + threadIdx.x;
  if (item >= nitems) return;
  const long s = item_s[item_base + item];
  const int c = item_c[item_base + item];
  const size_t o = (size_t)s + (size_t)c * (size_t)snps;
  const FirthFit a = fit[item];
  flag[o] = 2;
  if (a.status != kSpaSolved) return;
  const double e = __ddiv_rn(1.0, __dsqrt_rn(a.k2));
  double x2 = 2.0 * (a.beta * score[(size_t)s + (size_t)c * (size_t)ldu] - a.K);
  if (penalty) x2 += log(a.k2 / a.k20);
  if (!isfinite(e) || !isfinite(x2)) return;
  x2 = fmax(x2, 0.0);
  flag[o] = 1;
  beta[o] = a.beta;
  se[o] = e;
  chisq[o] = x2;
  pval[o] = erfc(sqrt(0.5 * x2));
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
    int p_dev = -1;
    in_place = ptr_location(plink, &p_dev) == 1 && p_dev == dev;   // rows in this device's memory are scanned where they lie
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

// ---- the stage of mxa_assoc_score_spa and mxa_assoc_score_firth after the scan: what the entries take beyond mxa_assoc_score's arguments.  penalty < 0: the
// saddlepoint correction (pval required); penalty 0 / 1: the fit (beta required; se, chisq and pval optional)
struct SpaArgs {
  const double *P;
  long ldp;
  double z_cutoff, tol;
  int max_iter;
  double *pval;
  int *flag;
  int penalty = -1;
  double *beta = nullptr, *se = nullptr, *chisq = nullptr;
  bool firth() const { return penalty >= 0; }
};

// the items one batch may hold: MXA_ASSOC_SPA_ITEMS (read per call, for tests), else what fits 4 GiB of g (512 items, 1024 workgroups of k_assoc_spa, at a
// million individuals) -- the fit: 8 GiB, since k_assoc_firth has one workgroup an item and 512 of them leave half of the device's workgroup slots empty, cut
// down to a multiple of the kFirthResident workgroups the device holds at once, so that no launch ends in a second round of a few (measured);
// at least the n items of one SNP
constexpr long kFirthResident = 1024;   // 256 CUs x 4 workgroups of 4 waves at 114 VGPRs
long spa_batch_items(long indiv, int n, bool firth) {
  long items = (long)(((size_t)(firth ? 8 : 4) << 30) / (sizeof(double) * (size_t)indiv));
  if (firth && items > kFirthResident) items -= items % kFirthResident;
  const char *e = getenv("MXA_ASSOC_SPA_ITEMS");
  if (e && atol(e) > 0) items = atol(e);
  return std::max<long>(n, items);
}
// the marked SNPs of one batch: MXA_ASSOC_SPA_BATCH, else unlimited for rows read in place and what fits a bounce buffer of 256 MiB for a host matrix
long spa_batch_rows(long snps, long bps, bool in_place) {
  long rows = in_place ? snps : std::max<long>(1, (long)(((size_t)256 << 20) / (size_t)bps));
  const char *e = getenv("MXA_ASSOC_SPA_BATCH");
  if (e && atol(e) > 0) rows = atol(e);
  return std::min(rows, snps);
}
// device memory of the stage at its largest (every trait of every SNP marked): the pre-flight's share
// (own: the snps x n arrays U, V, z that the stage allocates for itself; firth: beta, se and chisq beside pval, one FirthFit an item)
size_t spa_bytes(long snps, long indiv, int n, int kh, long bps, bool in_place, int own, bool firth) {
  const size_t cells = (size_t)snps * (size_t)n;
  const size_t items = (size_t)std::min<long>(spa_batch_items(indiv, n, firth), (long)cells);
  return cells * ((firth ? 4 : 1) * sizeof(double) + sizeof(int)) + (size_t)snps * sizeof(int) + ((size_t)snps + 1) * sizeof(long) + cells * 2 * sizeof(int) +
         sizeof(double) * (size_t)indiv * (size_t)n * ((size_t)kh + 1) + items * (sizeof(double) * (size_t)indiv + (firth ? sizeof(FirthFit) : 2 * sizeof(SpaSide))) +
         (in_place ? 0 : (size_t)spa_batch_rows(snps, bps, false) * (size_t)bps) + (size_t)own * cells * sizeof(double);
}

// After k_assoc_score_finish on d's stream: dU, dV and dZ are the scan's score, var and zstat on the device (ld ldu; dV: the fit only).  One host wait reads the
// number of marked SNPs and items with the list and its offsets; where nothing is marked neither P nor H is touched and no further kernel is launched.  The two
// entries share everything but the classify epilogue, the solve and the combine: the list, the items, tau, the batches, the bounce rows and k_assoc_spa_form.
int spa_stage(AssocDriver &d, const unsigned char *plink, const SpaArgs &a, int kh, const double *dU, const double *dV, const double *dZ, long ldu, long ldo) {
  const long snps = d.snps, indiv = d.indiv, bps = d.bps;
  const int n = d.n;
  hipStream_t s = d.s;
  const size_t cells = (size_t)snps * (size_t)n;
  const bool firth = a.firth();
  XBuf bPv, bFl, bList, bOff, bCount;
  if (bPv.alloc(sizeof(double) * cells * (firth ? 4 : 1)) || bFl.alloc(sizeof(int) * cells) || bList.alloc(sizeof(int) * (size_t)snps) ||
      bOff.alloc(sizeof(long) * ((size_t)snps + 1)) || bCount.alloc(2 * sizeof(long))) return 1;
  double *dPv = (double *)bPv.p, *dBeta = dPv + cells, *dSe = dBeta + cells, *dChi = dSe + cells;   // (the three of the fit)
  int *dFl = (int *)bFl.p, *dList = (int *)bList.p;
  long *dOff = (long *)bOff.p;
  launch_in_block_chunks(((long)cells + 255) / 256, [&](unsigned nb, long b0) {
    if (firth) k_assoc_firth_classify<<<nb, 256, 0, s>>>(snps, n, dU, dV, dZ, ldu, a.z_cutoff, dBeta, dSe, dChi, dPv, dFl, b0);
    else k_assoc_spa_classify<<<nb, 256, 0, s>>>(snps, n, dZ, ldu, a.z_cutoff, dPv, dFl, b0);
  });
  k_assoc_spa_list<<<1, 256, 0, s>>>(snps, n, dFl, dList, dOff, (long *)bCount.p);
  MXA_HIP(hipGetLastError());
  long count[2] = {0, 0};
  std::vector<int> list((size_t)snps);
  std::vector<long> off((size_t)snps + 1);
  MXA_HIP(hipMemcpyAsync(count, bCount.p, sizeof(count), hipMemcpyDeviceToHost, s));
  MXA_HIP(hipMemcpyAsync(list.data(), dList, sizeof(int) * (size_t)snps, hipMemcpyDeviceToHost, s));
  MXA_HIP(hipMemcpyAsync(off.data(), dOff, sizeof(long) * ((size_t)snps + 1), hipMemcpyDeviceToHost, s));
  MXA_HIP(hipStreamSynchronize(s));             // the one wait of the stage (only the first count[0] entries of list and off mean anything)
  const long nk = count[0], nitems = count[1];
  XBuf bP, bHt, bItemS, bItemC, bG, bSide, bRows;
  if (nitems > 0) {
    const size_t col = sizeof(double) * (size_t)indiv;
    if (bP.alloc(col * (size_t)n) || bHt.alloc(col * (size_t)n * (size_t)kh) || bItemS.alloc(sizeof(int) * (size_t)nitems) || bItemC.alloc(sizeof(int) * (size_t)nitems))
      return 1;
    MXA_HIP(hipMemcpy2DAsync(bP.p, col, a.P, sizeof(double) * (size_t)a.ldp, col, (size_t)n, hipMemcpyDefault, s));
    const unsigned iblocks = (unsigned)((indiv + 255) / 256);
    if (kh > 0)
      k_assoc_spa_tau<<<dim3(iblocks, (unsigned)(n * kh)), 256, 0, s>>>(d.dB + (size_t)2 * (size_t)n * (size_t)indiv, d.dB + (size_t)n * (size_t)indiv, indiv, kh,
                                                                        (double *)bHt.p);
    launch_in_block_chunks((nk + 255) / 256, [&](unsigned nb, long b0) {
      k_assoc_spa_items<<<nb, 256, 0, s>>>(nk, snps, n, dFl, dList, dOff, (int *)bItemS.p, (int *)bItemC.p, b0);
    });
    MXA_HIP(hipGetLastError());
    const long max_items = std::min(spa_batch_items(indiv, n, firth), nitems), max_rows = std::min(spa_batch_rows(snps, bps, d.in_place), nk);
    if (bG.alloc(sizeof(double) * (size_t)max_items * (size_t)indiv) || bSide.alloc((firth ? sizeof(FirthFit) : 2 * sizeof(SpaSide)) * (size_t)max_items) ||
        (!d.in_place && bRows.alloc((size_t)max_rows * (size_t)bps))) return 1;
    for (long k0 = 0; k0 < nk;) {
      long k1 = k0 + 1;                         // one SNP's items always fit; further SNPs while the rows and the items do
      while (k1 < nk && k1 - k0 < max_rows && off[(size_t)k1 + 1] - off[(size_t)k0] <= max_items) k1++;
      const long items = off[(size_t)k1] - off[(size_t)k0];
      const uint8_t *d_rows = plink;
      if (!d.in_place) {                        // the marked rows of a host matrix, row by row (runs of neighbouring rows in one copy) into the bounce buffer
        for (long k = k0; k < k1;) {
          long e = k + 1;
          while (e < k1 && list[(size_t)e] == list[(size_t)e - 1] + 1) e++;
          MXA_HIP(hipMemcpyAsync((uint8_t *)bRows.p + (size_t)(k - k0) * (size_t)bps, plink + (size_t)list[(size_t)k] * (size_t)bps, (size_t)(e - k) * (size_t)bps,
                                 hipMemcpyDefault, s));
          k = e;
        }
        d_rows = (const uint8_t *)bRows.p;
      }
      const long tiles = (k1 - k0 + kSpaTile - 1) / kSpaTile;
      launch_in_block_chunks(tiles * (long)iblocks, [&](unsigned nb, long b0) {
        k_assoc_spa_form<<<nb, 256, 0, s>>>(d_rows, bps, d.in_place ? 0 : 1, indiv, snps, n, kh, dList, dOff, k0, k1, dFl, d.dCnt, d.dCnt + snps, d.dCnt + 2 * snps, d.dD,
                                            d.dM, (const double *)bHt.p, (double *)bG.p, (long)iblocks, b0);
      });
      launch_in_block_chunks(firth ? items : 2 * items, [&](unsigned nb, long b0) {
        if (firth)
          k_assoc_firth<<<nb, 256, 0, s>>>((const double *)bG.p, indiv, (const double *)bP.p, (const int *)bItemS.p, (const int *)bItemC.p, off[(size_t)k0], items, dU,
                                           ldu, a.penalty, a.tol, a.max_iter, (FirthFit *)bSide.p, b0);
        else
          k_assoc_spa<<<nb, 256, 0, s>>>((const double *)bG.p, indiv, (const double *)bP.p, (const int *)bItemS.p, (const int *)bItemC.p, off[(size_t)k0], items, dU,
                                         ldu, a.tol, a.max_iter, (SpaSide *)bSide.p, b0);
      });
      launch_in_block_chunks((items + 255) / 256, [&](unsigned nb, long b0) {
        if (firth)
          k_assoc_firth_combine<<<nb, 256, 0, s>>>(items, off[(size_t)k0], (const int *)bItemS.p, (const int *)bItemC.p, dU, ldu, (const FirthFit *)bSide.p, a.penalty,
                                                   snps, dBeta, dSe, dChi, dPv, dFl, b0);
        else
          k_assoc_spa_combine<<<nb, 256, 0, s>>>(items, off[(size_t)k0], (const int *)bItemS.p, (const int *)bItemC.p, dU, ldu, (const SpaSide *)bSide.p, snps, dPv, dFl,
                                                 b0);
      });
      MXA_HIP(hipGetLastError());
      k0 = k1;
    }
  }
  const size_t pcol = sizeof(double) * (size_t)snps, fcol = sizeof(int) * (size_t)snps;
  const struct { double *to; const double *from; } results[4] = {{a.pval, dPv}, {a.beta, dBeta}, {a.se, dSe}, {a.chisq, dChi}};
  for (int j = 0; j < (firth ? 4 : 1); j++)
    if (results[j].to) MXA_HIP(hipMemcpy2DAsync(results[j].to, sizeof(double) * (size_t)ldo, results[j].from, pcol, pcol, (size_t)n, hipMemcpyDefault, s));
  if (a.flag) MXA_HIP(hipMemcpy2DAsync(a.flag, sizeof(int) * (size_t)ldo, dFl, fcol, fcol, (size_t)n, hipMemcpyDefault, s));
  MXA_HIP(hipStreamSynchronize(s));             // the buffers of the stage are released on return
  return 0;
}

// B = [R | Wt | H]: column c of R, column n + c of Wt, columns 2 n + c kh + j of H belong to trait c.  spa: the stage of the saddlepoint correction or of the
// fit follows the epilogue
int assoc_score(const unsigned char *plink, long snps, long indiv, const double *R, long ldr, const double *Wt, long ldw, const double *H, long ldh, int n, int kh,
                double *score, double *var, double *zstat, long ldo, int *nobs, bool out_dev, const SpaArgs *spa = nullptr, const AssocAfterScan *after = nullptr) {
  const int ncols = n * (kh + 2);
  AssocDriver d(after ? after->who : !spa ? "mxa_assoc_score" : spa->firth() ? "mxa_assoc_score_firth" : "mxa_assoc_score_spa", snps, indiv, ncols, n, out_dev);
  double *const res[3] = {score, var, zstat};
  const size_t e_bytes = sizeof(double) * (size_t)snps * (size_t)n;
  size_t extra = e_bytes;
  if (after) extra += after->extra_bytes + (score ? 0 : e_bytes);
  if (spa) {
    int p_dev = -1;
    const int dev = select_device();
    if (dev < 0) return 1;
    const bool in_place = ptr_location(plink, &p_dev) == 1 && p_dev == dev;
    extra += spa_bytes(snps, indiv, n, kh, (indiv + 3) / 4, in_place, !score + !zstat + (spa->firth() && !var), spa->firth());
  }
  if (d.begin(plink, res, extra)) return 1;
  hipStream_t s = d.s;
  XBuf bE, bU, bV, bZ;
  if (bE.alloc(e_bytes)) return 1;
  const long ldu = out_dev ? ldo : snps;
  if (spa) {                                    // the stage reads U and z (the fit: and V) on the device, whether the caller asked for them or not
    if (!d.out_d[0]) { if (bU.alloc(sizeof(double) * (size_t)ldu * (size_t)n)) return 1; d.out_d[0] = (double *)bU.p; }
    if (spa->firth() && !d.out_d[1]) { if (bV.alloc(sizeof(double) * (size_t)ldu * (size_t)n)) return 1; d.out_d[1] = (double *)bV.p; }
    if (!d.out_d[2]) { if (bZ.alloc(sizeof(double) * (size_t)ldu * (size_t)n)) return 1; d.out_d[2] = (double *)bZ.p; }
  }
  if (after && !d.out_d[0]) { if (bU.alloc(sizeof(double) * (size_t)ldu * (size_t)n)) return 1; d.out_d[0] = (double *)bU.p; }   // a stage reads U on the device
  double *dE = (double *)bE.p;
  const size_t col = sizeof(double) * (size_t)indiv;
  double *dW = d.dB + (size_t)n * (size_t)indiv;
  MXA_HIP(hipMemcpy2DAsync(d.dB, col, R, sizeof(double) * (size_t)ldr, col, (size_t)n, hipMemcpyDefault, s));
  MXA_HIP(hipMemcpy2DAsync(dW, col, Wt, sizeof(double) * (size_t)ldw, col, (size_t)n, hipMemcpyDefault, s));
  if (kh > 0)
    MXA_HIP(hipMemcpy2DAsync(d.dB + (size_t)2 * (size_t)n * (size_t)indiv, col, H, sizeof(double) * (size_t)ldh, col, (size_t)n * (size_t)kh, hipMemcpyDefault, s));
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
  if (spa && spa_stage(d, plink, *spa, kh, d.out_d[0], d.out_d[1], d.out_d[2], ldu, ldo)) return 1;
  if (after) {
    const AssocScanView v = {snps, indiv, bps, n, kh, d.in_place, out_dev, s, d.dCnt, d.dCnt + snps, d.dCnt + 2 * snps, d.dD, d.dM, dW, d.out_d[0], ldu};
    if (after->run(after->self, v, plink)) return 1;
  }
  return d.copy_out(res, ldo, nobs);
}

}  // namespace

int assoc_score_then(const unsigned char *plink, long snps, long indiv, const double *R, long ldr, const double *Wt, long ldw, const double *H, long ldh, int n, int kh,
                     double *score, double *var, double *zstat, long ldo, int *nobs, bool out_dev, const AssocAfterScan &after) {
  return assoc_score(plink, snps, indiv, R, ldr, Wt, ldw, H, ldh, n, kh, score, var, zstat, ldo, nobs, out_dev, nullptr, &after);
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
  int given = 0, on_dev = 0;
  for (const double *p : {(const double *)beta, (const double *)se, (const double *)tstat})
    if (p) { given++; on_dev += ptr_location(p, nullptr) == 1; }
  if (on_dev != 0 && on_dev != given) { set_error(1, "%s: beta, se and tstat must be all host or all device pointers", who); return 1; }
  int prev = -1;
  (void)hipGetDevice(&prev);
  const int rc = assoc_linear(plink, snps, indiv, Y, ldy, n, Q, ldq, k, beta, se, tstat, ldo, nobs, dof, on_dev != 0);
  if (prev >= 0) (void)hipSetDevice(prev);
  return rc;
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
  int given = 0, on_dev = 0;
  for (const double *p : {(const double *)score, (const double *)var, (const double *)zstat})
    if (p) { given++; on_dev += ptr_location(p, nullptr) == 1; }
  if (on_dev != 0 && on_dev != given) { set_error(1, "%s: score, var and zstat must be all host or all device pointers", who); return 1; }
  int prev = -1;
  (void)hipGetDevice(&prev);
  const int rc = assoc_score(plink, snps, indiv, R, ldr, Wt, ldw, H, ldh, n, kh, score, var, zstat, ldo, nobs, on_dev != 0);
  if (prev >= 0) (void)hipSetDevice(prev);
  return rc;
}

extern "C" int mxa_assoc_score_spa(const unsigned char *plink, int snps, int indiv, const double *P, long ldp, const double *R, long ldr, const double *Wt, long ldw,
                                   const double *H, long ldh, int n, int kh, double z_cutoff, double tol, int max_iter, double *score, double *var, double *zstat,
                                   double *pval, long ldo, int *flag, int *nobs) {
  using namespace mxa;
  clear_error();
  const char *who = "mxa_assoc_score_spa";
  const char *bad = assoc_score_spa_args(plink, snps, indiv, P, ldp, R, ldr, Wt, ldw, H, ldh, n, kh, z_cutoff, tol, max_iter, score, var, zstat, pval, ldo);
  if (bad) { set_error(1, "%s: %s", who, bad); return 1; }
  int given = 0, on_dev = 0;
  for (const double *p : {(const double *)score, (const double *)var, (const double *)zstat, (const double *)pval})
    if (p) { given++; on_dev += ptr_location(p, nullptr) == 1; }
  if (on_dev != 0 && on_dev != given) { set_error(1, "%s: score, var, zstat and pval must be all host or all device pointers", who); return 1; }
  if (flag && (ptr_location(flag, nullptr) == 1) != (on_dev != 0)) { set_error(1, "%s: flag and pval must be both host or both device pointers", who); return 1; }
  int prev = -1;
  (void)hipGetDevice(&prev);
  const SpaArgs spa = {P, ldp, z_cutoff, tol, max_iter, pval, flag};
  const int rc = assoc_score(plink, snps, indiv, R, ldr, Wt, ldw, H, ldh, n, kh, score, var, zstat, ldo, nobs, on_dev != 0, &spa);
  if (prev >= 0) (void)hipSetDevice(prev);
  return rc;
}

extern "C" int mxa_assoc_score_firth(const unsigned char *plink, int snps, int indiv, const double *P, long ldp, const double *R, long ldr, const double *Wt, long ldw,
                                     const double *H, long ldh, int n, int kh, double z_cutoff, int penalty, double tol, int max_iter, double *score, double *var,
                                     double *zstat, double *beta, double *se, double *chisq, double *pval, long ldo, int *flag, int *nobs) {
  using namespace mxa;
  clear_error();
  const char *who = "mxa_assoc_score_firth";
  const char *bad = assoc_score_firth_args(plink, snps, indiv, P, ldp, R, ldr, Wt, ldw, H, ldh, n, kh, z_cutoff, penalty, tol, max_iter, score, var, zstat, beta, ldo);
  if (bad) { set_error(1, "%s: %s", who, bad); return 1; }
  int given = 0, on_dev = 0;
  for (const double *p : {(const double *)score, (const double *)var, (const double *)zstat, (const double *)beta, (const double *)se, (const double *)chisq,
                          (const double *)pval})
    if (p) { given++; on_dev += ptr_location(p, nullptr) == 1; }
  if (on_dev != 0 && on_dev != given) { set_error(1, "%s: score, var, zstat, beta, se, chisq and pval must be all host or all device pointers", who); return 1; }
  if (flag && (ptr_location(flag, nullptr) == 1) != (on_dev != 0)) { set_error(1, "%s: flag and beta must be both host or both device pointers", who); return 1; }
  int prev = -1;
  (void)hipGetDevice(&prev);
  SpaArgs fit = {P, ldp, z_cutoff, tol, max_iter, pval, flag};
  fit.penalty = penalty;
  fit.beta = beta;
  fit.se = se;
  fit.chisq = chisq;
  const int rc = assoc_score(plink, snps, indiv, R, ldr, Wt, ldw, H, ldh, n, kh, score, var, zstat, ldo, nobs, on_dev != 0, &fit);
  if (prev >= 0) (void)hipSetDevice(prev);
  return rc;
}
