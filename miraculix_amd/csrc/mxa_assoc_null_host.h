// mxa_assoc_null_host.h -- the host-only null model of the score test (mxa_assoc_logistic_null; the scan is mxa_assoc_score in mxa_assoc.hip): logistic
// regression of a 0 / 1 trait on C = [1 | W] by Newton / IRLS, and what the scan needs from it -- the residual, the working weight and the projection columns
// H = diag(w) C L^-T.  Plain C++ without any HIP header (tools/assoc_score_host_check.cpp compiles it for the CPU under -fsanitize=address,undefined).
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace mxa {

constexpr int kAssocNullHalvings = 20;   // a Newton step is halved at most this often while the deviance rises

// Returns 0, or 2: column *bad of W holds a non-finite entry; 3: y[*bad] is not exactly 0 or 1; 4: all y are equal; 5: C^T diag(w) C is not positive definite
// at column *bad of C (0 = the intercept, j = column j - 1 of W): a pivot of the Cholesky factorisation is at most indiv 2^-52 times its diagonal entry; 6: no
// convergence within max_iter steps, or a step that 20 halvings did not make descend (separation).  Sums are carried in long double.  gamma (q + 1), r, w
// (indiv each), H (indiv x (q + 1), ld ldh) and *iters (optional) are written only on success.  Every work array is allocated before the first output
// is written: std::bad_alloc leaves the outputs untouched (the caller catches it).
inline int assoc_logistic_null_host(long indiv, const double *y, const double *W, long ldw, int q, double tol, int max_iter, double *gamma, double *r, double *w,
                                    double *H, long ldh, int *iters, long *bad) {
  typedef long double real;
  const int p = q + 1;
  const size_t n = (size_t)indiv;
  long cases = 0;
  for (long i = 0; i < indiv; i++) {
    if (!(y[i] == 0.0 || y[i] == 1.0)) { *bad = i; return 3; }
    cases += y[i] == 1.0;
  }
  for (int j = 0; j < q; j++)
    for (long i = 0; i < indiv; i++)
      if (!std::isfinite(W[(size_t)j * (size_t)ldw + (size_t)i])) { *bad = j; return 2; }
  if (cases == 0 || cases == indiv) return 4;
  auto c_at = [&](long i, int j) -> real { return j == 0 ? (real)1 : (real)W[(size_t)(j - 1) * (size_t)ldw + (size_t)i]; };
  std::vector<real> g((size_t)p, (real)0), trial((size_t)p), delta((size_t)p), A((size_t)p * (size_t)p), L((size_t)p * (size_t)p), rhs((size_t)p), x((size_t)p);
  std::vector<real> eta(n), prob(n);
  // eta = C g, prob = 1 / (1 + exp(-eta)); returns the deviance 2 sum softplus((1 - 2 y) eta)
  auto evaluate = [&](const std::vector<real> &gam) -> real {
    real dev = 0;
    for (long i = 0; i < indiv; i++) {
      real e = 0;
      for (int j = 0; j < p; j++) e += c_at(i, j) * gam[(size_t)j];
      eta[(size_t)i] = e;
      prob[(size_t)i] = e >= 0 ? (real)1 / ((real)1 + std::exp(-e)) : std::exp(e) / ((real)1 + std::exp(e));
      const real v = y[i] == 1.0 ? -e : e;
      dev += v > 0 ? v + std::log1p(std::exp(-v)) : std::log1p(std::exp(v));
    }
    return 2 * dev;
  };
  // A = C^T diag(prob (1 - prob)) C and its lower Cholesky factor L; 0, or 5 with *bad = the column
  auto factor = [&]() -> int {
    for (size_t t = 0; t < A.size(); t++) A[t] = 0;
    for (long i = 0; i < indiv; i++) {
      const real wi = prob[(size_t)i] * ((real)1 - prob[(size_t)i]);
      for (int a = 0; a < p; a++) {
        const real wa = wi * c_at(i, a);
        for (int b = 0; b <= a; b++) A[(size_t)a * (size_t)p + (size_t)b] += wa * c_at(i, b);
      }
    }
    for (int a = 0; a < p; a++) {
      for (int b = 0; b <= a; b++) {
        real s = A[(size_t)a * (size_t)p + (size_t)b];
        for (int k = 0; k < b; k++) s -= L[(size_t)a * (size_t)p + (size_t)k] * L[(size_t)b * (size_t)p + (size_t)k];
        if (a == b) {
          if (!(s > (real)indiv * 0x1p-52L * A[(size_t)a * (size_t)p + (size_t)a])) { *bad = a; return 5; }
          L[(size_t)a * (size_t)p + (size_t)a] = std::sqrt(s);
        } else {
          L[(size_t)a * (size_t)p + (size_t)b] = s / L[(size_t)b * (size_t)p + (size_t)b];
        }
      }
    }
    return 0;
  };
  const real ybar = (real)cases / (real)indiv;
  g[0] = std::log(ybar / ((real)1 - ybar));
  real dev = evaluate(g);
  int it = 0;
  bool converged = false;
  while (it < max_iter && !converged) {
    it++;
    if (factor()) {
      // weights that vanished because a fitted probability ran into 0 or 1 (|eta| > 30) are the separated problem on its way to infinity, not a bad column
      real emax = 0;
      for (long i = 0; i < indiv; i++) emax = std::fmax(emax, std::fabs(eta[(size_t)i]));
      return it > 1 && emax > 30 ? 6 : 5;
    }
    for (int a = 0; a < p; a++) {
      real s = 0;
      for (long i = 0; i < indiv; i++) s += c_at(i, a) * ((real)y[i] - prob[(size_t)i]);
      rhs[(size_t)a] = s;
    }
    for (int a = 0; a < p; a++) {            // L u = rhs, then L^T delta = u
      real s = rhs[(size_t)a];
      for (int k = 0; k < a; k++) s -= L[(size_t)a * (size_t)p + (size_t)k] * delta[(size_t)k];
      delta[(size_t)a] = s / L[(size_t)a * (size_t)p + (size_t)a];
    }
    for (int a = p - 1; a >= 0; a--) {
      real s = delta[(size_t)a];
      for (int k = a + 1; k < p; k++) s -= L[(size_t)k * (size_t)p + (size_t)a] * delta[(size_t)k];
      delta[(size_t)a] = s / L[(size_t)a * (size_t)p + (size_t)a];
    }
    real step = 1;
    int halvings = 0;
    for (;;) {
      for (int a = 0; a < p; a++) trial[(size_t)a] = g[(size_t)a] + step * delta[(size_t)a];
      const real d = evaluate(trial);
      if (d <= dev + dev * 0x1p-50L) { dev = d; break; }      // a rise at the rounding level of the sum is none; a non-finite deviance compares false: halve
      if (++halvings > kAssocNullHalvings) return 6;
      step /= 2;
    }
    real dmax = 0, gmax = 0;
    for (int a = 0; a < p; a++) {
      dmax = std::fmax(dmax, std::fabs(step * delta[(size_t)a]));
      g[(size_t)a] = trial[(size_t)a];
      gmax = std::fmax(gmax, std::fabs(g[(size_t)a]));
    }
    converged = dmax <= (real)tol * std::fmax((real)1, gmax);
  }
  if (!converged) return 6;
  // eta and prob belong to g (the accepted trial was evaluated last); the factor of the final weights gives H
  if (factor()) return 5;
  for (int a = 0; a < p; a++) gamma[a] = (double)g[(size_t)a];
  for (long i = 0; i < indiv; i++) {
    const real pi = prob[(size_t)i], wi = pi * ((real)1 - pi);
    r[i] = (double)((real)y[i] - pi);
    w[i] = (double)wi;
    for (int a = 0; a < p; a++) {            // L x = c_i
      real s = c_at(i, a);
      for (int k = 0; k < a; k++) s -= L[(size_t)a * (size_t)p + (size_t)k] * x[(size_t)k];
      x[(size_t)a] = s / L[(size_t)a * (size_t)p + (size_t)a];
      H[(size_t)a * (size_t)ldh + (size_t)i] = (double)(wi * x[(size_t)a]);
    }
  }
  if (iters) *iters = it;
  return 0;
}

// The argument rules of mxa_assoc_logistic_null: nullptr when they hold, else what is wrong.  No pointer is dereferenced.
inline const char *assoc_logistic_null_args(long indiv, const void *y, const void *W, long ldw, int q, const void *gamma, const void *r, const void *w, const void *H,
                                            long ldh) {
  if (indiv < 1 || q < 0) return "indiv must be positive and q must not be negative";
  if (!y || !gamma || !r || !w || !H) return "y, gamma, r, w and H must not be NULL";
  if (q > 0 && !W) return "W is NULL with q > 0";
  if (indiv <= (long)q + 1) return "indiv must exceed q + 1";
  if ((q > 0 && ldw < indiv) || ldh < indiv) return "ldw and ldh must be at least indiv";
  return nullptr;
}

}  // namespace mxa
