// mxa_assoc_stage.h -- what a unit of its own shares with the association scan (mxa_assoc.hip): the decode convention of the raw PLINK rows (the logical
// 16-byte words of assoc_load_word: the same fields for every alignment of a row) and the way a stage follows the score scan on the scan's own stream and
// buffers, as the saddlepoint stage and the Firth fit do inside mxa_assoc.hip.  mxa_assoc_set.hip (the set tests) is its user.
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

// What the scan leaves on the device for a stage that follows k_assoc_score_finish on stream s.  Columns of D and M (ld snps): c = R, n + c = Wt,
// 2 n + c kh + j = H; a_jh of SNP s and trait c is fma(mu, M, D) at s + (2 n + c kh + h) snps with mu = (c1 + 2 c2) / N.  W: the working weights, indiv x n,
// ld indiv.  U: the scores, ld ldu.  in_place: plink is memory of the scan's device and is read where it lies.
struct AssocScanView {
  long snps, indiv, bps;
  int n, kh;
  bool in_place, out_dev;
  hipStream_t s;
  const int *nobs, *c1, *c2;
  const double *D, *M, *W, *U;
  long ldu;
};

// A stage after the scan: run() enqueues on v.s and returns after its own last wait (0, or 1 with the error set); extra_bytes joins the scan's memory pre-flight.
struct AssocAfterScan {
  const char *who;
  size_t extra_bytes;
  void *self;
  int (*run)(void *self, const AssocScanView &v, const unsigned char *plink);
};

// mxa_assoc_score's scan with every result optional, then the stage (mxa_assoc.hip)
int assoc_score_then(const unsigned char *plink, long snps, long indiv, const double *R, long ldr, const double *Wt, long ldw, const double *H, long ldh, int n, int kh,
                     double *score, double *var, double *zstat, long ldo, int *nobs, bool out_dev, const AssocAfterScan &after);

}  // namespace mxa
