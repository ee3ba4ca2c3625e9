// Stand-alone check of the host-only part of the association scan (miraculix_amd/csrc/mxa_assoc_host.h: the covariate basis of mxa_assoc_basis, the argument
// rules of mxa_assoc_linear), for a CPU build under sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/assoc_host_check.cpp -o assoc_host_check && ./assoc_host_check
// The operands are heap blocks of exactly the bytes the entry may touch (the last column ends at row indiv - 1), so a read or write past them is reported.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>
#include "../miraculix_amd/csrc/mxa_assoc_host.h"

static int fail(const char *what, long indiv, int q, long at) {
  std::printf("FAIL: %s (indiv %ld, q %d, at %ld)\n", what, indiv, q, at);
  return 1;
}

int main() {
  std::mt19937_64 rng(20250611);
  std::normal_distribution<double> normal(0.0, 1.0);
  for (int trial = 0; trial < 300; trial++) {
    const long indiv = 3 + (long)(rng() % 200);
    const int q = 1 + (int)(rng() % std::min<long>(12, indiv - 2));
    const long ldw = indiv + (long)(rng() % 4), ldq = indiv + (long)(rng() % 4);
    std::vector<double> W((size_t)ldw * (size_t)(q - 1) + (size_t)indiv), Q((size_t)ldq * (size_t)(q - 1) + (size_t)indiv, -7.5);
    for (int j = 0; j < q; j++) {
      const double scale = 0.5 + (double)(rng() % 40), shift = 200.0 * normal(rng);
      for (long i = 0; i < ldw && (size_t)j * (size_t)ldw + (size_t)i < W.size(); i++)
        W[(size_t)j * (size_t)ldw + (size_t)i] = i < indiv ? shift + scale * normal(rng) : std::numeric_limits<double>::quiet_NaN();   // the rows behind a column are not read
    }
    int bad = -1;
    if (mxa::assoc_basis_host(indiv, W.data(), ldw, q, Q.data(), ldq, &bad) != 0) return fail("a full-rank W was refused", indiv, q, bad);
    const long double tol = 8.0L * (long double)indiv * 0x1p-53L;
    for (int a = 0; a < q; a++) {
      long double sum = 0.0L;
      for (long i = 0; i < indiv; i++) sum += Q[(size_t)a * (size_t)ldq + (size_t)i];
      if (std::fabs(sum) > tol) return fail("a column does not sum to zero", indiv, q, a);
      for (int b = 0; b <= a; b++) {
        long double dot = 0.0L;
        for (long i = 0; i < indiv; i++) dot += (long double)Q[(size_t)a * (size_t)ldq + (size_t)i] * Q[(size_t)b * (size_t)ldq + (size_t)i];
        if (std::fabs(dot - (a == b ? 1.0L : 0.0L)) > tol) return fail("Q^T Q != I", indiv, q, a * 100 + b);
      }
      for (long i = indiv; i < ldq && (size_t)a * (size_t)ldq + (size_t)i < Q.size(); i++)
        if (Q[(size_t)a * (size_t)ldq + (size_t)i] != -7.5) return fail("a row behind a column of Q was written", indiv, q, a);
      // column a of the centred W lies in the span of the columns 0 .. a of Q: its residual after the projection is rounding
      std::vector<long double> r((size_t)indiv);
      long double mean = 0.0L, top = 0.0L;
      for (long i = 0; i < indiv; i++) mean += W[(size_t)a * (size_t)ldw + (size_t)i];
      mean /= (long double)indiv;
      for (long i = 0; i < indiv; i++) { r[(size_t)i] = W[(size_t)a * (size_t)ldw + (size_t)i] - mean; top = std::fmax(top, std::fabs(r[(size_t)i])); }
      for (int b = 0; b <= a; b++) {
        long double dot = 0.0L;
        for (long i = 0; i < indiv; i++) dot += r[(size_t)i] * Q[(size_t)b * (size_t)ldq + (size_t)i];
        for (long i = 0; i < indiv; i++) r[(size_t)i] -= dot * Q[(size_t)b * (size_t)ldq + (size_t)i];
      }
      for (long i = 0; i < indiv; i++)
        if (std::fabs(r[(size_t)i]) > 64.0L * tol * top) return fail("the centred W is not in the span of Q", indiv, q, a);
    }
    // a broken column -- constant, a multiple of the column before it, or one non-finite entry -- is named and leaves Q as it was
    std::vector<double> keep = Q, Wb = W;
    const int b = (int)(rng() % (unsigned)q), kind = (int)(rng() % 3);
    int want = 3;
    if (kind == 0) for (long i = 0; i < indiv; i++) Wb[(size_t)b * (size_t)ldw + (size_t)i] = 4.25;
    else if (kind == 1 && b > 0) for (long i = 0; i < indiv; i++) Wb[(size_t)b * (size_t)ldw + (size_t)i] = -2.0 * Wb[(size_t)(b - 1) * (size_t)ldw + (size_t)i];   // (exactly dependent: no rounding in the data)
    else if (kind == 1) for (long i = 0; i < indiv; i++) Wb[(size_t)i] = -1.0;
    else { Wb[(size_t)b * (size_t)ldw + (size_t)(rng() % (unsigned long)indiv)] = rng() % 2 ? INFINITY : std::numeric_limits<double>::quiet_NaN(); want = 2; }
    bad = -1;
    if (mxa::assoc_basis_host(indiv, Wb.data(), ldw, q, Q.data(), ldq, &bad) != want || bad != b) return fail("a broken column was not named", indiv, q, b);
    if (Q != keep) return fail("Q was written by a refused call", indiv, q, b);
  }
  // the argument rules of mxa_assoc_linear: no pointer is dereferenced
  const void *p = &rng;
  if (mxa::assoc_linear_args(p, 5, 12, p, 12, 2, p, 12, 3, p, nullptr, nullptr, 5) != nullptr) return fail("valid arguments were refused", 12, 3, 0);
  if (mxa::assoc_linear_args(p, 5, 12, p, 12, 2, nullptr, 0, 0, nullptr, nullptr, p, 5) != nullptr) return fail("k = 0 with a NULL Q was refused", 12, 0, 0);
  const char *refused[] = {
      mxa::assoc_linear_args(nullptr, 5, 12, p, 12, 2, p, 12, 3, p, p, p, 5), mxa::assoc_linear_args(p, 5, 12, nullptr, 12, 2, p, 12, 3, p, p, p, 5),
      mxa::assoc_linear_args(p, 0, 12, p, 12, 2, p, 12, 3, p, p, p, 5),       mxa::assoc_linear_args(p, 5, 0, p, 12, 2, p, 12, 3, p, p, p, 5),
      mxa::assoc_linear_args(p, 5, 12, p, 12, 0, p, 12, 3, p, p, p, 5),       mxa::assoc_linear_args(p, 5, 12, p, 12, 2, p, 12, -1, p, p, p, 5),
      mxa::assoc_linear_args(p, 5, 12, p, 12, 2, nullptr, 12, 3, p, p, p, 5), mxa::assoc_linear_args(p, 5, 12, p, 11, 2, p, 12, 3, p, p, p, 5),
      mxa::assoc_linear_args(p, 5, 12, p, 12, 2, p, 11, 3, p, p, p, 5),       mxa::assoc_linear_args(p, 5, 12, p, 12, 2, p, 12, 3, p, p, p, 4),
      mxa::assoc_linear_args(p, 5, 12, p, 12, 2, p, 12, 10, p, p, p, 5),      mxa::assoc_linear_args(p, 5, 12, p, 12, 2, p, 12, 3, nullptr, nullptr, nullptr, 5),
      mxa::assoc_linear_args(p, 5, 70000, p, 70000, 65535, p, 70000, 1, p, p, p, 5),
      mxa::assoc_linear_args(p, 5, mxa::kAssocMaxIndiv + 1, p, mxa::kAssocMaxIndiv + 1, 2, p, mxa::kAssocMaxIndiv + 1, 3, p, p, p, 5)};
  for (size_t i = 0; i < sizeof(refused) / sizeof(refused[0]); i++)
    if (!refused[i]) return fail("invalid arguments were accepted", 12, 3, (long)i);
  if (mxa::assoc_linear_args(p, 5, mxa::kAssocMaxIndiv, p, mxa::kAssocMaxIndiv, 2, p, mxa::kAssocMaxIndiv, 3, p, p, p, 5) != nullptr) return fail("the largest indiv was refused", 0, 0, 0);
  std::printf("assoc_host_check: PASS\n");
  return 0;
}
