// Stand-alone check of the host-only part of the score test (miraculix_amd/csrc/mxa_assoc_null_host.h: the logistic null model of mxa_assoc_logistic_null and its
// argument rules; miraculix_amd/csrc/mxa_assoc_host.h: the argument rules of mxa_assoc_score), for a CPU build under sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan tools/assoc_score_host_check.cpp \
//       -o assoc_score_host_check && ./assoc_score_host_check
// (the runtimes linked statically: the program is self-contained and runs in whatever environment it is started in)
// The operands are heap blocks of exactly the bytes the entry may touch (the last column ends at row indiv - 1), so a read or write past them is reported.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>
#include "../miraculix_amd/csrc/mxa_assoc_host.h"
#include "../miraculix_amd/csrc/mxa_assoc_null_host.h"

static int fail(const char *what, long indiv, int q, long at) {
  std::printf("FAIL: %s (indiv %ld, q %d, at %ld)\n", what, indiv, q, at);
  return 1;
}

struct Fit {
  std::vector<double> gamma, r, w, H;
  int iters = -3;
};

int main() {
  std::mt19937_64 rng(20250619);
  std::normal_distribution<double> normal(0.0, 1.0);
  std::uniform_real_distribution<double> uniform(0.0, 1.0);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int trial = 0; trial < 200; trial++) {
    const int q = trial % 4 == 0 ? 0 : 1 + (int)(rng() % 4);
    const long indiv = 60 + 30 * q + (long)(rng() % 200);
    const long ldw = indiv + (long)(rng() % 4), ldh = indiv + (long)(rng() % 4);
    const int p = q + 1;
    std::vector<double> y((size_t)indiv), W(q ? (size_t)ldw * (size_t)(q - 1) + (size_t)indiv : 0);
    for (int j = 0; j < q; j++)
      for (long i = 0; i < ldw && (size_t)j * (size_t)ldw + (size_t)i < W.size(); i++)
        W[(size_t)j * (size_t)ldw + (size_t)i] = i < indiv ? 1.5 + normal(rng) : nan;   // the rows behind a column are not read
    for (long i = 0; i < indiv; i++) {
      double eta = -0.4;
      for (int j = 0; j < q; j++) eta += 0.3 * (W[(size_t)j * (size_t)ldw + (size_t)i] - 1.5);
      y[(size_t)i] = uniform(rng) < 1.0 / (1.0 + std::exp(-eta)) ? 1.0 : 0.0;
    }
    y[0] = 1.0;
    y[1] = 0.0;
    Fit f;
    f.gamma.assign((size_t)p, -7.5);
    f.r.assign((size_t)indiv, -7.5);
    f.w.assign((size_t)indiv, -7.5);
    f.H.assign((size_t)ldh * (size_t)(p - 1) + (size_t)indiv, -7.5);
    const double *Wp = q ? W.data() : nullptr;
    if (mxa::assoc_logistic_null_args(indiv, y.data(), Wp, ldw, q, f.gamma.data(), f.r.data(), f.w.data(), f.H.data(), ldh)) return fail("valid arguments were refused", indiv, q, 0);
    long bad = -1;
    const int rc = mxa::assoc_logistic_null_host(indiv, y.data(), Wp, ldw, q, 1e-10, 50, f.gamma.data(), f.r.data(), f.w.data(), f.H.data(), ldh, &f.iters, &bad);
    if (rc != 0) return fail("a regular problem was refused", indiv, q, rc);
    if (f.iters < 1 || f.iters > 50) return fail("iters", indiv, q, f.iters);
    // the score equations C^T r = 0, r = y - p, w = p (1 - p); C^T H is lower triangular with a positive diagonal and (C^T H)(C^T H)^T = C^T diag(w) C
    auto c_at = [&](long i, int j) -> long double { return j == 0 ? 1.0L : (long double)W[(size_t)(j - 1) * (size_t)ldw + (size_t)i]; };
    std::vector<long double> A((size_t)p * (size_t)p, 0.0L), Lm((size_t)p * (size_t)p, 0.0L);
    for (int a = 0; a < p; a++) {
      long double s = 0.0L, scale = 0.0L;
      for (long i = 0; i < indiv; i++) { s += c_at(i, a) * f.r[(size_t)i]; scale += std::fabs(c_at(i, a)); }
      if (std::fabs(s) > 1e-9L * scale) return fail("C^T r != 0", indiv, q, a);
      for (int b = 0; b < p; b++)
        for (long i = 0; i < indiv; i++) {
          A[(size_t)a * (size_t)p + (size_t)b] += c_at(i, a) * f.w[(size_t)i] * c_at(i, b);
          Lm[(size_t)a * (size_t)p + (size_t)b] += c_at(i, a) * f.H[(size_t)b * (size_t)ldh + (size_t)i];
        }
    }
    for (long i = 0; i < indiv; i++) {
      const double pi = y[(size_t)i] - f.r[(size_t)i];
      if (!(pi > 0.0 && pi < 1.0) || std::fabs(f.w[(size_t)i] - pi * (1.0 - pi)) > 1e-15) return fail("r or w", indiv, q, i);
    }
    for (int a = 0; a < p; a++)
      for (int b = 0; b < p; b++) {
        const long double tol = 1e-12L * std::sqrt(A[(size_t)a * (size_t)p + (size_t)a] * A[(size_t)b * (size_t)p + (size_t)b]);
        if (b > a && std::fabs(Lm[(size_t)a * (size_t)p + (size_t)b]) > 1e-10L * std::sqrt(A[(size_t)a * (size_t)p + (size_t)a])) return fail("C^T H is not lower triangular", indiv, q, a * 100 + b);
        if (b == a && !(Lm[(size_t)a * (size_t)p + (size_t)a] > 0.0L)) return fail("the diagonal of C^T H is not positive", indiv, q, a);
        long double s = 0.0L;
        for (int k = 0; k < p; k++) s += Lm[(size_t)a * (size_t)p + (size_t)k] * Lm[(size_t)b * (size_t)p + (size_t)k];
        if (std::fabs(s - A[(size_t)a * (size_t)p + (size_t)b]) > tol) return fail("(C^T H)(C^T H)^T != C^T W C", indiv, q, a * 100 + b);
      }
    for (int a = 0; a < p; a++)
      for (long i = indiv; i < ldh && (size_t)a * (size_t)ldh + (size_t)i < f.H.size(); i++)
        if (f.H[(size_t)a * (size_t)ldh + (size_t)i] != -7.5) return fail("a row behind a column of H was written", indiv, q, a);
    // every error path leaves the outputs as they were
    const Fit keep = f;
    auto untouched = [&]() { return f.gamma == keep.gamma && f.r == keep.r && f.w == keep.w && f.H == keep.H && f.iters == keep.iters; };
    auto refit = [&](const std::vector<double> &yy, const std::vector<double> &WW, int max_iter, int want, long want_bad) {
      long b = -1;
      const int got = mxa::assoc_logistic_null_host(indiv, yy.data(), q ? WW.data() : nullptr, ldw, q, 1e-10, max_iter, f.gamma.data(), f.r.data(), f.w.data(), f.H.data(),
                                                    ldh, &f.iters, &b);
      return got == want && (want_bad < 0 || b == want_bad) && untouched();
    };
    std::vector<double> yb = y;
    const long at = (long)(rng() % (unsigned long)indiv);
    yb[(size_t)at] = trial % 2 ? 0.5 : nan;
    if (!refit(yb, W, 50, 3, at)) return fail("a y that is not 0 or 1 was not named", indiv, q, at);
    std::fill(yb.begin(), yb.end(), trial % 2 ? 1.0 : 0.0);
    if (!refit(yb, W, 50, 4, -1)) return fail("an all-equal y was accepted", indiv, q, 0);
    if (!refit(y, W, 0, 6, -1)) return fail("max_iter = 0 did not report no convergence", indiv, q, 0);
    if (q > 0) {
      const int col = (int)(rng() % (unsigned)q);
      std::vector<double> Wb = W;
      Wb[(size_t)col * (size_t)ldw + (size_t)(rng() % (unsigned long)indiv)] = trial % 2 ? INFINITY : nan;
      if (!refit(y, Wb, 50, 2, col)) return fail("a non-finite covariate was not named", indiv, q, col);
      Wb = W;
      for (long i = 0; i < indiv; i++) Wb[(size_t)col * (size_t)ldw + (size_t)i] = col > 0 && trial % 2 ? -2.0 * Wb[(size_t)(col - 1) * (size_t)ldw + (size_t)i] : 4.25;
      if (!refit(y, Wb, 50, 5, col + 1)) return fail("a constant or dependent column was not named", indiv, q, col);
      Wb = W;
      for (long i = 0; i < indiv; i++) Wb[(size_t)col * (size_t)ldw + (size_t)i] = y[(size_t)i];     // separation: the covariate is the trait
      long b = -1;
      const int got = mxa::assoc_logistic_null_host(indiv, y.data(), Wb.data(), ldw, q, 1e-10, 50, f.gamma.data(), f.r.data(), f.w.data(), f.H.data(), ldh, &f.iters, &b);
      if ((got != 5 && got != 6) || !untouched()) return fail("a separated problem was accepted", indiv, q, got);
    }
  }
  // the argument rules: no pointer is dereferenced
  const void *p = &rng;
  if (mxa::assoc_logistic_null_args(12, p, nullptr, 0, 0, p, p, p, p, 12) != nullptr) return fail("q = 0 with a NULL W was refused", 12, 0, 0);
  const char *null_refused[] = {
      mxa::assoc_logistic_null_args(0, p, p, 12, 2, p, p, p, p, 12),        mxa::assoc_logistic_null_args(12, p, p, 12, -1, p, p, p, p, 12),
      mxa::assoc_logistic_null_args(12, nullptr, p, 12, 2, p, p, p, p, 12), mxa::assoc_logistic_null_args(12, p, nullptr, 12, 2, p, p, p, p, 12),
      mxa::assoc_logistic_null_args(12, p, p, 12, 2, nullptr, p, p, p, 12), mxa::assoc_logistic_null_args(12, p, p, 12, 2, p, nullptr, p, p, 12),
      mxa::assoc_logistic_null_args(12, p, p, 12, 2, p, p, nullptr, p, 12), mxa::assoc_logistic_null_args(12, p, p, 12, 2, p, p, p, nullptr, 12),
      mxa::assoc_logistic_null_args(12, p, p, 11, 2, p, p, p, p, 12),       mxa::assoc_logistic_null_args(12, p, p, 12, 2, p, p, p, p, 11),
      mxa::assoc_logistic_null_args(3, p, p, 3, 2, p, p, p, p, 3)};
  for (size_t i = 0; i < sizeof(null_refused) / sizeof(null_refused[0]); i++)
    if (!null_refused[i]) return fail("invalid arguments of the null model were accepted", 12, 2, (long)i);
  const long big = mxa::kAssocMaxIndiv;
  if (mxa::assoc_score_args(p, 5, 12, p, 12, p, 12, p, 12, 2, 3, p, nullptr, nullptr, 5) != nullptr) return fail("valid arguments were refused", 12, 3, 0);
  if (mxa::assoc_score_args(p, 5, 12, p, 12, p, 12, nullptr, 0, 2, 0, nullptr, nullptr, p, 5) != nullptr) return fail("kh = 0 with a NULL H was refused", 12, 0, 0);
  if (mxa::assoc_score_args(p, 5, big, p, big, p, big, p, big, 2, 3, p, p, p, 5) != nullptr) return fail("the largest indiv was refused", 0, 0, 0);
  if (mxa::assoc_score_args(p, 5, 12, p, 12, p, 12, p, 12, 65535 / 5, 3, p, p, p, 5) != nullptr) return fail("n (kh + 2) = 65535 was refused", 0, 0, 0);
  const char *refused[] = {
      mxa::assoc_score_args(nullptr, 5, 12, p, 12, p, 12, p, 12, 2, 3, p, p, p, 5), mxa::assoc_score_args(p, 5, 12, nullptr, 12, p, 12, p, 12, 2, 3, p, p, p, 5),
      mxa::assoc_score_args(p, 5, 12, p, 12, nullptr, 12, p, 12, 2, 3, p, p, p, 5), mxa::assoc_score_args(p, 0, 12, p, 12, p, 12, p, 12, 2, 3, p, p, p, 5),
      mxa::assoc_score_args(p, 5, 0, p, 12, p, 12, p, 12, 2, 3, p, p, p, 5),        mxa::assoc_score_args(p, 5, 12, p, 12, p, 12, p, 12, 0, 3, p, p, p, 5),
      mxa::assoc_score_args(p, 5, 12, p, 12, p, 12, p, 12, 2, -1, p, p, p, 5),      mxa::assoc_score_args(p, 5, 12, p, 12, p, 12, nullptr, 12, 2, 3, p, p, p, 5),
      mxa::assoc_score_args(p, 5, 12, p, 11, p, 12, p, 12, 2, 3, p, p, p, 5),       mxa::assoc_score_args(p, 5, 12, p, 12, p, 11, p, 12, 2, 3, p, p, p, 5),
      mxa::assoc_score_args(p, 5, 12, p, 12, p, 12, p, 11, 2, 3, p, p, p, 5),       mxa::assoc_score_args(p, 5, 12, p, 12, p, 12, p, 12, 2, 3, p, p, p, 4),
      mxa::assoc_score_args(p, 5, 12, p, 12, p, 12, p, 12, 2, 3, nullptr, nullptr, nullptr, 5),
      mxa::assoc_score_args(p, 5, 12, p, 12, p, 12, p, 12, 65535 / 5 + 1, 3, p, p, p, 5),
      mxa::assoc_score_args(p, 5, big + 1, p, big + 1, p, big + 1, p, big + 1, 2, 3, p, p, p, 5)};
  for (size_t i = 0; i < sizeof(refused) / sizeof(refused[0]); i++)
    if (!refused[i]) return fail("invalid arguments of the scan were accepted", 12, 3, (long)i);
  std::printf("assoc_score_host_check: PASS\n");
  return 0;
}
