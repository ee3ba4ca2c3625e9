// mxa_assoc_host.h -- the host-only part of the association scan (mxa_assoc.hip) and of its saddlepoint / Firth stage (mxa_assoc_spa.hip): the covariate basis of
// mxa_assoc_basis and the argument rules of mxa_assoc_linear, mxa_assoc_score, mxa_assoc_score_spa and mxa_assoc_score_firth (the null model of the score test: mxa_assoc_null_host.h).  Plain C++ without any HIP header, so that a stand-alone
// program can compile it for the CPU (tools/assoc_host_check.cpp, tools/assoc_score_host_check.cpp, tools/assoc_firth_host_check.cpp, run under
// -fsanitize=address,undefined).
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace mxa {

constexpr long kAssocMaxIndiv = 47453132L;   // 4 indiv^2 < 2^53: the numerator N Szz - Sz^2 of a SNP's variance is an exact integer in fp64
constexpr int kAssocCols = 16;               // columns of B = [Y~ | Q] one pass of the scan carries (one packed row: 16 doubles of one individual)

// Q (indiv x q, ld ldq) = an orthonormal, zero-sum basis of the centred columns of W (indiv x q, ld ldw), in place order: column j is W's column j minus its
// mean, made orthogonal to the columns before it by Gram-Schmidt applied twice (every pass ends with a centring, so that the column sums stay at rounding
// level), then scaled to norm 1.  Sums are carried in long double.  Q is written only when every column passed.
// Returns 0, or 2: a non-finite entry (*bad = its column), 3: column *bad is constant or depends on the columns before it -- its norm after the two passes
// is at most indiv 2^-52 times its centred norm.
inline int assoc_basis_host(long indiv, const double *W, long ldw, int q, double *Q, long ldq, int *bad) {
  std::vector<double> out((size_t)indiv * (size_t)q);
  std::vector<long double> v((size_t)indiv);
  auto centre = [&]() {
    long double s = 0.0L;
    for (long i = 0; i < indiv; i++) s += v[(size_t)i];
    const long double mean = s / (long double)indiv;
    for (long i = 0; i < indiv; i++) v[(size_t)i] -= mean;
  };
  auto norm = [&]() {
    long double s = 0.0L;
    for (long i = 0; i < indiv; i++) s += v[(size_t)i] * v[(size_t)i];
    return std::sqrt(s);
  };
  for (int j = 0; j < q; j++) {
    const double *w = W + (size_t)j * (size_t)ldw;
    for (long i = 0; i < indiv; i++) {
      if (!std::isfinite(w[i])) { *bad = j; return 2; }
      v[(size_t)i] = w[i];
    }
    centre();
    const long double norm0 = norm();
    for (int pass = 0; pass < 2; pass++) {
      for (int p = 0; p < j; p++) {
        const double *qp = out.data() + (size_t)p * (size_t)indiv;
        long double dot = 0.0L;
        for (long i = 0; i < indiv; i++) dot += (long double)qp[i] * v[(size_t)i];
        for (long i = 0; i < indiv; i++) v[(size_t)i] -= dot * (long double)qp[i];
      }
      centre();
    }
    const long double nrm = norm();
    if (!(nrm > (long double)indiv * 0x1p-52L * norm0)) { *bad = j; return 3; }
    double *o = out.data() + (size_t)j * (size_t)indiv;
    for (long i = 0; i < indiv; i++) o[i] = (double)(v[(size_t)i] / nrm);
  }
  for (int j = 0; j < q; j++)
    for (long i = 0; i < indiv; i++) Q[(size_t)j * (size_t)ldq + (size_t)i] = out[(size_t)j * (size_t)indiv + (size_t)i];
  return 0;
}

// The argument rules of mxa_assoc_linear that need no device: nullptr when they hold, else what is wrong.  (Mixed host / device result pointers are the
// caller's check: it needs the runtime's pointer attributes.)
inline const char *assoc_linear_args(const void *plink, long snps, long indiv, const void *Y, long ldy, int n, const void *Q, long ldq, int k, const void *beta,
                                     const void *se, const void *tstat, long ldo) {
  if (!plink || !Y) return "plink and Y must not be NULL";
  if (snps < 1 || indiv < 1 || n < 1) return "snps, indiv and n must be positive";
  if (k < 0) return "k must not be negative";
  if ((long)n + (long)k > 65535) return "n + k must be at most 65535";
  if (k > 0 && !Q) return "Q is NULL with k > 0";
  if (ldy < indiv || (k > 0 && ldq < indiv)) return "ldy and ldq must be at least indiv";
  if (indiv - (long)k - 2 < 1) return "indiv - k - 2 degrees of freedom must be at least 1";
  if (indiv > kAssocMaxIndiv) return "indiv > 47 453 132 (4 indiv^2 >= 2^53)";
  if (!beta && !se && !tstat) return "beta, se and tstat are all NULL";
  if (ldo < snps) return "ldo must be at least snps";
  return nullptr;
}

// The same for mxa_assoc_score: B = [R | Wt | H] has n (kh + 2) columns.
inline const char *assoc_score_args(const void *plink, long snps, long indiv, const void *R, long ldr, const void *Wt, long ldw, const void *H, long ldh, int n, int kh,
                                    const void *score, const void *var, const void *zstat, long ldo, bool need_result = true) {
  if (!plink || !R || !Wt) return "plink, R and Wt must not be NULL";
  if (snps < 1 || indiv < 1 || n < 1) return "snps, indiv and n must be positive";
  if (kh < 0) return "kh must not be negative";
  if (kh > 0 && !H) return "H is NULL with kh > 0";
  if ((long)n * ((long)kh + 2) > 65535) return "n (kh + 2) must be at most 65535";
  if (ldr < indiv || ldw < indiv || (kh > 0 && ldh < indiv)) return "ldr, ldw and ldh must be at least indiv";
  if (indiv > kAssocMaxIndiv) return "indiv > 47 453 132 (4 indiv^2 >= 2^53)";
  if (need_result && !score && !var && !zstat) return "score, var and zstat are all NULL";   // (mxa_assoc_set: its set results are the point)
  if (ldo < snps) return "ldo must be at least snps";
  return nullptr;
}

// The same for mxa_assoc_score_spa: mxa_assoc_score's rules, then its own.  (flag and pval on different sides are the caller's check.)
inline const char *assoc_score_spa_args(const void *plink, long snps, long indiv, const void *P, long ldp, const void *R, long ldr, const void *Wt, long ldw,
                                        const void *H, long ldh, int n, int kh, double z_cutoff, double tol, int max_iter, const void *score, const void *var,
                                        const void *zstat, const void *pval, long ldo) {
  if (const char *bad = assoc_score_args(plink, snps, indiv, R, ldr, Wt, ldw, H, ldh, n, kh, score, var, zstat, ldo)) return bad;
  if (!P || !pval) return "P and pval must not be NULL";
  if (ldp < indiv) return "ldp must be at least indiv";
  if (!(z_cutoff >= 0.0)) return "z_cutoff must not be negative or NaN";
  if (!(tol > 0.0 && tol < 1.0)) return "tol must lie in (0, 1)";
  if (max_iter < 1) return "max_iter must be at least 1";
  return nullptr;
}

// The same for mxa_assoc_score_firth: mxa_assoc_score_spa's rules with beta in pval's place, then its own.  (Mixed sides among the results are the caller's check.)
inline const char *assoc_score_firth_args(const void *plink, long snps, long indiv, const void *P, long ldp, const void *R, long ldr, const void *Wt, long ldw,
                                          const void *H, long ldh, int n, int kh, double z_cutoff, int penalty, double tol, int max_iter, const void *score,
                                          const void *var, const void *zstat, const void *beta, long ldo) {
  if (const char *bad = assoc_score_args(plink, snps, indiv, R, ldr, Wt, ldw, H, ldh, n, kh, score, var, zstat, ldo)) return bad;
  if (!P || !beta) return "P and beta must not be NULL";
  if (const char *bad = assoc_score_spa_args(plink, snps, indiv, P, ldp, R, ldr, Wt, ldw, H, ldh, n, kh, z_cutoff, tol, max_iter, score, var, zstat, beta, ldo)) return bad;
  if (penalty != 0 && penalty != 1) return "penalty must be 0 or 1";
  return nullptr;
}

}  // namespace mxa
