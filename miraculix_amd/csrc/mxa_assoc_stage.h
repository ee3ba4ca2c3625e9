// mxa_assoc_stage.h -- what the units of the association family share with the scan (mxa_assoc.hip): the decode convention of the raw PLINK rows (the logical
// 16-byte words of assoc_load_word: the same fields for every alignment of a row; assoc_mu and assoc_decode: the value of a field), the workgroup sum tree
// (assoc_block_sums) and the way a stage follows the score scan on the scan's own stream and buffers (AssocScanView, AssocAfterScan, assoc_score_then).  The
// stages: mxa_assoc_spa.hip (the saddlepoint correction and the Firth fit) and mxa_assoc_set.hip (the set tests).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace mxa {

struct AssocWord { unsigned long long lo, hi; };

// Logical word w of a row: its bytes [16 w, 16 w + 16) below bps, the rest zero.  Only aligned 16-byte words that hold at least one byte of the row are
// loaded: such a word lies in the page of that byte, so nothing unmapped is touched even where it reaches before the first row or behind the last one.
__device__ __forceinline__ AssocWord assoc_load_word(const uint8_t *__restrict__ row, long w, long bps, int sh) {
  const long b0 = 16 * w, nb = bps - b0;                          // nb >= 1 bytes of the row from b0 on
  const uint4 *a = reinterpret_cast<const uint4 *>(row + b0 - sh);
  const uint4 x = a[0];
  uint4 y = make_uint4(0u, 0u, 0u, 0u);
  if (sh && 16 - sh < nb) y = a[1];                               // the logical word reaches into the next aligned one
  const unsigned long long q0 = (unsigned long long)x.x | ((unsigned long long)x.y << 32), q1 = (unsigned long long)x.z | ((unsigned long long)x.w << 32);
  const unsigned long long q2 = (unsigned long long)y.x | ((unsigned long long)y.y << 32), q3 = (unsigned long long)y.z | ((unsigned long long)y.w << 32);
  const bool big = sh >= 8;
  const int s8 = 8 * (sh & 7);
  const unsigned long long A = big ? q1 : q0, B = big ? q2 : q1, C = big ? q3 : q2;
  AssocWord r;
  r.lo = s8 ? (A >> s8) | (B << (64 - s8)) : A;
  r.hi = s8 ? (B >> s8) | (C << (64 - s8)) : B;
  if (nb < 16) {                                                  // the row ends inside this word: what follows belongs to the next row, or to nobody
    if (nb <= 8) { r.hi = 0ull; if (nb < 8) r.lo &= (1ull << (8 * nb)) - 1ull; }
    else r.hi &= (1ull << (8 * (nb - 8))) - 1ull;
  }
  return r;
}

// mu of SNP s, the value of its missing calls: (c1 + 2 c2) / N, as k_assoc_score_finish forms it
__device__ __forceinline__ double assoc_mu(const int *__restrict__ nobs, const int *__restrict__ c1, const int *__restrict__ c2, long s) {
  return __ddiv_rn((double)((long)c1[s] + 2 * (long)c2[s]), (double)nobs[s]);
}
__device__ __forceinline__ double assoc_decode(unsigned code, double mu) {        // 00 -> 0, 01 -> mu, 10 -> 1, 11 -> 2
  return (code & 2u) ? ((code & 1u) ? 2.0 : 1.0) : ((code & 1u) ? mu : 0.0);
}

// K sums of a workgroup of 256 threads at once: a fixed tree -- the wave's shuffles (32, 16, ..., 1), then (w0 + w1) + (w2 + w3) through the LDS -- so the
// order depends on nothing but what every thread brings.  Every thread returns with the K totals; red may be used again at once.
template <int K>
__device__ __forceinline__ void assoc_block_sums(double (&v)[K], double (*red)[4]) {
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

// What the scan leaves on the device for a stage that follows k_assoc_score_finish on stream s.  Columns of D and M (ld snps): c = R, n + c = Wt,
// 2 n + c kh + j = H; a_jh of SNP s and trait c is fma(mu, M, D) at s + (2 n + c kh + h) snps with mu = (c1 + 2 c2) / N.  W: the working weights, indiv x n,
// ld indiv; H: the n kh columns of H, ld indiv.  U, V, Z: the scores, variances and z statistics, ld ldu -- each is there only where the stage states that it
// reads it (or the caller asked for it).  in_place: plink is memory of the scan's device and is read where it lies.
struct AssocScanView {
  long snps, indiv, bps;
  int n, kh;
  bool in_place, out_dev;
  hipStream_t s;
  const int *nobs, *c1, *c2;
  const double *D, *M, *W, *H, *U, *V, *Z;
  long ldu;
};

// A stage after the scan: run() enqueues on v.s and returns after its own last wait (0, or 1 with the error set).  reads: which of score, var and zstat the
// stage reads on the device -- the scan keeps an array of its own for each of them that the caller did not give and counts its snps x n doubles in the memory
// pre-flight; extra_bytes: what the stage allocates itself, joins that pre-flight too.
struct AssocAfterScan {
  const char *who;
  size_t extra_bytes;
  bool reads[3];
  void *self;
  int (*run)(void *self, const AssocScanView &v, const unsigned char *plink);
};

// mxa_assoc_score's scan with every result optional, then the stage (mxa_assoc.hip)
int assoc_score_then(const unsigned char *plink, long snps, long indiv, const double *R, long ldr, const double *Wt, long ldw, const double *H, long ldh, int n, int kh,
                     double *score, double *var, double *zstat, long ldo, int *nobs, bool out_dev, const AssocAfterScan &after);

}  // namespace mxa
