// mxa_assoc_set_host.h -- the host-only part of the set tests (mxa_assoc_set.hip): the argument rules and the CSR validation of mxa_assoc_set, the plan of its
// batches, and mxa_assoc_skat_pvalue.  Plain C++ without any HIP header, so that a stand-alone program can compile it for the CPU
// (tools/assoc_set_host_check.cpp, run under -fsanitize=address,undefined).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <limits>
#include <vector>
#include "mxa_assoc_host.h"

namespace mxa {

constexpr int kSetTile = 16;        // edge of a Gram tile: one v_mfma_f64_16x16x4_f64 result
constexpr long kSetSplit = 4096;    // individuals of one piece of the split: 64 logical words of 64 genotypes, 16 for each of a workgroup's four waves
constexpr long kSetMaxSize = 1024;  // entries of one set: Phi of one (set, trait) is at most 8 MiB
constexpr size_t kSetBudget = (size_t)1 << 30;   // bytes of S / Phi and of the partial sums one batch may take by default (one set always fits)

inline long set_tiles(long m) { return (m + kSetTile - 1) / kSetTile; }
inline long set_pairs(long m) { const long t = set_tiles(m); return t * (t + 1) / 2; }     // tile pairs j <= j'
inline long set_pieces(long indiv) { return (indiv + kSetSplit - 1) / kSetSplit; }

// The argument rules of mxa_assoc_set that need no device: 0 when they hold, else 1 with what is wrong in msg.  (Mixed host / device result pointers are the
// caller's check.)
inline int assoc_set_args(const void *plink, long snps, long indiv, const void *R, long ldr, const void *Wt, long ldw, const void *H, long ldh, int n, int kh,
                          int nsets, const long *set_ptr, const int *set_idx, const void *score, const void *var, const void *zstat, long ldo, const void *stat,
                          long lds, char *msg, size_t msg_len) {
  if (const char *bad = assoc_score_args(plink, snps, indiv, R, ldr, Wt, ldw, H, ldh, n, kh, score, var, zstat, ldo, false)) { snprintf(msg, msg_len, "%s", bad); return 1; }
  if (nsets < 1) { snprintf(msg, msg_len, "nsets must be positive"); return 1; }
  if (!set_ptr || !set_idx || !stat) { snprintf(msg, msg_len, "set_ptr, set_idx and stat must not be NULL"); return 1; }
  if (lds < nsets) { snprintf(msg, msg_len, "lds must be at least nsets"); return 1; }
  if (set_ptr[0] != 0) { snprintf(msg, msg_len, "set_ptr[0] must be 0"); return 1; }
  for (int k = 0; k < nsets; k++) {
    const long m = set_ptr[k + 1] - set_ptr[k];
    if (m < 0) { snprintf(msg, msg_len, "set_ptr decreases at set %d", k); return 1; }
    if (m > kSetMaxSize) { snprintf(msg, msg_len, "set %d has %ld entries: at most %ld", k, m, kSetMaxSize); return 1; }
  }
  for (int k = 0; k < nsets; k++)
    for (long e = set_ptr[k]; e < set_ptr[k + 1]; e++)
      if (set_idx[e] < 0 || (long)set_idx[e] >= snps) {
        snprintf(msg, msg_len, "entry %ld of set %d is the SNP %d: outside [0, %ld)", e - set_ptr[k], k, set_idx[e], snps);
        return 1;
      }
  return 0;
}

// ---- the batches: consecutive sets, cut by entries (max_entries; never below one whole set) and by the byte budget of S / Phi and the partial sums
struct SetBatch {
  int k0, k1;            // sets [k0, k1)
  long entries, descs, items, tiles;   // set entries; (set, trait, tile pair) work items; (set, trait) items; the tiles of all items
  size_t phi_doubles;    // n sum m^2
};
inline size_t set_batch_bytes(const SetBatch &b, long pieces) {
  return sizeof(double) * (b.phi_doubles + (size_t)b.descs * (size_t)pieces * (size_t)(kSetTile * kSetTile) + 3 * (size_t)b.tiles);
}
inline std::vector<SetBatch> set_plan(int nsets, const long *set_ptr, int n, long indiv, long max_entries, size_t budget) {
  std::vector<SetBatch> plan;
  const long pieces = set_pieces(indiv);
  SetBatch cur = {0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < nsets; k++) {
    const long m = set_ptr[k + 1] - set_ptr[k];
    SetBatch with = cur;
    with.k1 = k + 1;
    with.entries += m;
    with.descs += (long)n * set_pairs(m);
    with.items += n;
    with.tiles += (long)n * set_tiles(m);
    with.phi_doubles += (size_t)n * (size_t)m * (size_t)m;
    if (cur.k1 > cur.k0 && (with.entries > max_entries || set_batch_bytes(with, pieces) > budget)) {
      plan.push_back(cur);
      cur = {k, k, 0, 0, 0, 0, 0};
      k--;
      continue;
    }
    cur = with;
  }
  plan.push_back(cur);
  return plan;
}

// ---- mxa_assoc_skat_pvalue: Q = sum lambda_i chi^2_1 matched to a central chi-square by c1 = tr A, c2 = tr A^2, c4 = tr A^4 (Liu's recipe in its modified
// form; for a positive semi-definite A its non-central branch is never taken): l = c2^2 / c4, x = (Q - c1) sqrt(l / c2) + l, p = Q(l / 2, x / 2), the
// regularised upper incomplete gamma function, and 1 where x <= 0.  Sums in long double on the log scale: the series of P for x < a + 1, else the continued
// fraction of Q (modified Lentz).
inline long double skat_gamma_q(long double a, long double x) {
  const long double eps = 0x1p-63L;
  if (x < a + 1.0L) {
    long double term = 1.0L, sum = 1.0L, ap = a;
    for (int it = 0; it < 100000; it++) {
      ap += 1.0L;
      term *= x / ap;
      sum += term;
      if (term <= sum * eps) break;
    }
    const long double P = sum * expl(a * logl(x) - x - lgammal(a + 1.0L));
    return 1.0L - P;
  }
  const long double tiny = std::numeric_limits<long double>::min() * 0x1p64L;
  long double b = x + 1.0L - a, c = 1.0L / tiny, d = 1.0L / b, h = d;
  for (int i = 1; i < 100000; i++) {
    const long double an = -(long double)i * ((long double)i - a);
    b += 2.0L;
    d = an * d + b;
    if (fabsl(d) < tiny) d = tiny;
    c = b + an / c;
    if (fabsl(c) < tiny) c = tiny;
    d = 1.0L / d;
    const long double del = d * c;
    h *= del;
    if (fabsl(del - 1.0L) <= eps) break;
  }
  return h * expl(a * logl(x) - x - lgammal(a));
}

// one item: the p-value, *df = l (NaN with it where the moments are not those of a non-zero positive semi-definite A)
inline double skat_pvalue_host(double Q, double c1, double c2, double c4, double *df) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (!std::isfinite(Q) || !std::isfinite(c1) || !std::isfinite(c2) || !std::isfinite(c4) || !(c2 > 0.0) || !(c4 > 0.0)) { if (df) *df = nan; return nan; }
  const long double l = ((long double)c2 * (long double)c2) / (long double)c4;
  const long double x = ((long double)Q - (long double)c1) * sqrtl(l / (long double)c2) + l;
  if (!std::isfinite((double)l) || !(l > 0.0L) || std::isnan(x)) { if (df) *df = nan; return nan; }
  if (df) *df = (double)l;
  if (x <= 0.0L) return 1.0;
  const long double p = skat_gamma_q(0.5L * l, 0.5L * x);
  return p < 0.0L ? 0.0 : p > 1.0L ? 1.0 : (double)p;
}

}  // namespace mxa
