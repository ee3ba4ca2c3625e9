// mxa_assoc_spa.hip -- the stage of mxa_assoc_score_spa and mxa_assoc_score_firth (include/miraculix_amd.h): the saddlepoint correction
// of the score test's p-values and the (Firth-penalised) fit of the SNP's effect, for the SNPs with |z| >= z_cutoff.  The scan runs unchanged (mxa_assoc.hip:
// assoc_score_then); this unit is the stage that follows it on the scan's stream and reads the scan's buffers through an AssocScanView (mxa_assoc_stage.h).
// The two entries share everything but the classify epilogue, the solve and the combine.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <vector>
#include "../../include/miraculix_amd.h"
#include "mxa_internal.h"
#include "mxa_assoc_host.h"
#include "mxa_assoc_stage.h"
#include "mxa_xprod.h"

namespace mxa {

namespace {

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
// marked SNPs from k0 + kSpaTile tile on.  Every thread decodes its field of each of these rows once (assoc_decode with the SNP's
// assoc_mu), then per trait c with an item in the tile reads tau_{c,j,i} once per j and applies it to all of the tile's SNPs with that item:
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
      mu[u] = assoc_mu(nobs, c1, c2, s[u]);
      if (live) {
        const uint8_t *row = rows + (size_t)(compact ? k - k0 : s[u]) * (size_t)bps;
        x[u] = assoc_decode((row[i >> 2] >> (2 * (int)(i & 3))) & 3u, mu[u]);
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

// ---- what the two solves (k_assoc_spa, k_assoc_firth) share.  The first pass over row g of G: c0 = sum g p (an FMA chain), A = sum |g|, G+ and G-; every
// thread returns with the four totals.
__device__ __forceinline__ void spa_first_sums(const double *__restrict__ g, const double *__restrict__ p, long indiv, double (&v4)[4], double (*red)[4]) {
#pragma unroll
  for (int q = 0; q < 4; q++) v4[q] = 0.0;
  for (long i = threadIdx.x; i < indiv; i += 256) {
    const double gi = g[i];
    v4[0] = __fma_rn(gi, p[i], v4[0]);
    v4[1] += fabs(gi);
    v4[2] += fmax(gi, 0.0);
    v4[3] += fmin(gi, 0.0);
  }
  assoc_block_sums<4>(v4, red);
}

// One term of an evaluation at the point t: x = t g, e = exp(-|x|), and with (al, be) = (p, 1 - p) for x >= 0, (1 - p, p) otherwise, d = al + be e and r = 1 / d
// -- one exp and one division a term, K' and K'' take the reciprocal.
struct SpaTerm { double x, e, al, be, d, r; bool pos; };
__device__ __forceinline__ SpaTerm spa_term(double t, double gi, double pi) {
  SpaTerm m;
  m.x = t * gi;
  m.e = exp(-fabs(m.x));
  m.pos = m.x >= 0.0;
  m.al = m.pos ? pi : 1.0 - pi;
  m.be = m.pos ? 1.0 - pi : pi;
  m.d = m.al + m.be * m.e;
  m.r = 1.0 / m.d;
  return m;
}

// The safeguarded Newton step (thread 0) after evaluation number `evals` at t gave the value f and the slope fp: the bracket takes t, tn = t - f / fp; a tn
// that is not finite fails, one within tol of t is accepted, one outside the bracket is replaced by the bracket's middle, and the step fails when that is not
// finite or max_iter evaluations are spent.
constexpr int kNewtonFailed = 0, kNewtonAccepted = 1, kNewtonGoOn = 2;
__device__ __forceinline__ int spa_newton_step(double f, double fp, double t, double &lo, double &hi, double tol, int max_iter, int evals, double &tn) {
  if (f < 0.0) lo = t; else hi = t;
  tn = t - f / fp;
  if (!isfinite(tn)) return kNewtonFailed;
  if (fabs(tn - t) <= tol * fabs(tn)) return kNewtonAccepted;
  if (!(tn > lo && tn < hi)) tn = 0.5 * (lo + hi);
  if (!isfinite(tn) || evals >= max_iter) return kNewtonFailed;
  return kNewtonGoOn;
}

// (b) one workgroup per (item, side): item = blk0 + blockIdx.x >> 1 of the batch (row `item` of G), side 0: sigma = +1, side 1: sigma = -1.  Thread t takes the
// individuals t, t + 256, ... in ascending order; every sum ends in assoc_block_sums, so its order depends on indiv alone.  First c0, A, G+ and G-, then Newton
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
  double v4[4];
  spa_first_sums(g, p, indiv, v4, red);
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
      const SpaTerm m = spa_term(t, gi, pi);
      if (state == 1) v3[0] += fmax(m.x, 0.0) + log(m.d);
      else v3[1] += gi * ((m.pos ? pi : pi * m.e) * m.r);
      v3[2] += (gi * m.r) * (gi * m.r) * (m.al * m.be * m.e);
    }
    assoc_block_sums<3>(v3, red);
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
        double tn;
        const int step = spa_newton_step((v3[1] - c0) - q, v3[2], t, lo, hi, tol, max_iter, evals, tn);
        if (step == kNewtonFailed) status = kSpaFailed;
        else { sh_t = tn; if (step == kNewtonAccepted) sh_state = 1; }
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
// assoc_block_sums, so its order depends on indiv alone.  First c0, A, G+ and G- (penalty == 0: the support test of the observed side), then Newton from beta = 0
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
  double v4[4];
  spa_first_sums(g, p, indiv, v4, red);
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
      const SpaTerm m = spa_term(b, gi, pi);
      const double r = m.r, gr = gi * r, abe = m.al * m.be * m.e, t2 = gr * gr * abe;   // t2 = g^2 omega
      if (state == 1) v2[0] += fmax(m.x, 0.0) + log(m.d);
      else {
        const double pr = (m.pos ? pi : pi * m.e) * r;
        v2[0] += gi * pr;
        if (penalty) {
          const double t3 = t2 * gi;
          w2[0] = fma(t3, 1.0 - 2.0 * pr, w2[0]);
          w2[1] = fma(t3 * gi, 1.0 - 6.0 * (abe * r * r), w2[1]);
        }
      }
      v2[1] += t2;
    }
    assoc_block_sums<2>(v2, red);
    if (penalty && state == 0) assoc_block_sums<2>(w2, red);
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
        double bn;
        const int step = spa_newton_step(f, fp, b, lo, hi, tol, max_iter, evals, bn);
        if (step == kNewtonFailed) status = kSpaFailed;
        else { sh_b = bn; if (step == kNewtonAccepted) sh_state = 1; }
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

// ---- host side: what the entries take beyond mxa_assoc_score's arguments (ldo: of pval, flag, beta, se and chisq).  penalty < 0: the saddlepoint correction
// (pval required); penalty 0 / 1: the fit (beta required; se, chisq and pval optional)
struct SpaArgs {
  const double *P;
  long ldp;
  double z_cutoff, tol;
  int max_iter;
  double *pval;
  int *flag;
  long ldo;
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
// (firth: beta, se and chisq beside pval, one FirthFit an item)
size_t spa_bytes(long snps, long indiv, int n, int kh, long bps, bool in_place, bool firth) {
  const size_t cells = (size_t)snps * (size_t)n;
  const size_t items = (size_t)std::min<long>(spa_batch_items(indiv, n, firth), (long)cells);
  return cells * ((firth ? 4 : 1) * sizeof(double) + sizeof(int)) + (size_t)snps * sizeof(int) + ((size_t)snps + 1) * sizeof(long) + cells * 2 * sizeof(int) +
         sizeof(double) * (size_t)indiv * (size_t)n * ((size_t)kh + 1) + items * (sizeof(double) * (size_t)indiv + (firth ? sizeof(FirthFit) : 2 * sizeof(SpaSide))) +
         (in_place ? 0 : (size_t)spa_batch_rows(snps, bps, false) * (size_t)bps);
}

// After k_assoc_score_finish on the scan's stream: v.U, v.V and v.Z are the scan's score, var and zstat on the device (v.V: the fit only).  One host wait reads the
// number of marked SNPs and items with the list and its offsets; where nothing is marked neither P nor H is touched and no further kernel is launched.  The two
// entries share everything but the classify epilogue, the solve and the combine: the list, the items, tau, the batches, the bounce rows and k_assoc_spa_form.
int spa_stage(const AssocScanView &v, const unsigned char *plink, const SpaArgs &a) {
  const long snps = v.snps, indiv = v.indiv, bps = v.bps, ldu = v.ldu, ldo = a.ldo;
  const int n = v.n, kh = v.kh;
  const double *dU = v.U, *dV = v.V, *dZ = v.Z;
  hipStream_t s = v.s;
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
      k_assoc_spa_tau<<<dim3(iblocks, (unsigned)(n * kh)), 256, 0, s>>>(v.H, v.W, indiv, kh, (double *)bHt.p);
    launch_in_block_chunks((nk + 255) / 256, [&](unsigned nb, long b0) {
      k_assoc_spa_items<<<nb, 256, 0, s>>>(nk, snps, n, dFl, dList, dOff, (int *)bItemS.p, (int *)bItemC.p, b0);
    });
    MXA_HIP(hipGetLastError());
    const long max_items = std::min(spa_batch_items(indiv, n, firth), nitems), max_rows = std::min(spa_batch_rows(snps, bps, v.in_place), nk);
    if (bG.alloc(sizeof(double) * (size_t)max_items * (size_t)indiv) || bSide.alloc((firth ? sizeof(FirthFit) : 2 * sizeof(SpaSide)) * (size_t)max_items) ||
        (!v.in_place && bRows.alloc((size_t)max_rows * (size_t)bps))) return 1;
    for (long k0 = 0; k0 < nk;) {
      long k1 = k0 + 1;                         // one SNP's items always fit; further SNPs while the rows and the items do
      while (k1 < nk && k1 - k0 < max_rows && off[(size_t)k1 + 1] - off[(size_t)k0] <= max_items) k1++;
      const long items = off[(size_t)k1] - off[(size_t)k0];
      const uint8_t *d_rows = plink;
      if (!v.in_place) {                        // the marked rows of a host matrix into the bounce buffer
        if (assoc_gather_rows((uint8_t *)bRows.p, plink, bps, list.data() + k0, k1 - k0, s)) return 1;
        d_rows = (const uint8_t *)bRows.p;
      }
      const long tiles = (k1 - k0 + kSpaTile - 1) / kSpaTile;
      launch_in_block_chunks(tiles * (long)iblocks, [&](unsigned nb, long b0) {
        k_assoc_spa_form<<<nb, 256, 0, s>>>(d_rows, bps, v.in_place ? 0 : 1, indiv, snps, n, kh, dList, dOff, k0, k1, dFl, v.nobs, v.c1, v.c2, v.D, v.M,
                                            (const double *)bHt.p, (double *)bG.p, (long)iblocks, b0);
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

int spa_stage_run(void *self, const AssocScanView &v, const unsigned char *plink) { return spa_stage(v, plink, *static_cast<const SpaArgs *>(self)); }

// what both entries do after their argument checks: the scan with the stage behind it.  The stage reads U and z (the fit: and V) on the device, whether the
// caller asked for them or not.
int score_then_stage(const char *who, const unsigned char *plink, long snps, long indiv, const double *R, long ldr, const double *Wt, long ldw, const double *H, long ldh,
                     int n, int kh, double *score, double *var, double *zstat, long ldo, int *nobs, bool out_dev, SpaArgs &a) {
  DeviceRestore restore;
  const int dev = select_device();
  if (dev < 0) return 1;
  const long bps = (indiv + 3) / 4;
  const AssocAfterScan after = {who, spa_bytes(snps, indiv, n, kh, bps, assoc_rows_in_place(plink, dev), a.firth()), {true, a.firth(), true}, &a, spa_stage_run};
  return assoc_score_then(plink, snps, indiv, R, ldr, Wt, ldw, H, ldh, n, kh, score, var, zstat, ldo, nobs, out_dev, after);
}

}  // namespace

}  // namespace mxa

extern "C" int mxa_assoc_score_spa(const unsigned char *plink, int snps, int indiv, const double *P, long ldp, const double *R, long ldr, const double *Wt, long ldw,
                                   const double *H, long ldh, int n, int kh, double z_cutoff, double tol, int max_iter, double *score, double *var, double *zstat,
                                   double *pval, long ldo, int *flag, int *nobs) {
  using namespace mxa;
  clear_error();
  const char *who = "mxa_assoc_score_spa";
  const char *bad = assoc_score_spa_args(plink, snps, indiv, P, ldp, R, ldr, Wt, ldw, H, ldh, n, kh, z_cutoff, tol, max_iter, score, var, zstat, pval, ldo);
  if (bad) { set_error(1, "%s: %s", who, bad); return 1; }
  bool out_dev = false;
  if (results_on_one_side(who, "score, var, zstat and pval", {score, var, zstat, pval}, &out_dev)) return 1;
  if (flag && (ptr_location(flag, nullptr) == 1) != out_dev) { set_error(1, "%s: flag and pval must be both host or both device pointers", who); return 1; }
  SpaArgs spa = {P, ldp, z_cutoff, tol, max_iter, pval, flag, ldo};
  return score_then_stage(who, plink, snps, indiv, R, ldr, Wt, ldw, H, ldh, n, kh, score, var, zstat, ldo, nobs, out_dev, spa);
}

extern "C" int mxa_assoc_score_firth(const unsigned char *plink, int snps, int indiv, const double *P, long ldp, const double *R, long ldr, const double *Wt, long ldw,
                                     const double *H, long ldh, int n, int kh, double z_cutoff, int penalty, double tol, int max_iter, double *score, double *var,
                                     double *zstat, double *beta, double *se, double *chisq, double *pval, long ldo, int *flag, int *nobs) {
  using namespace mxa;
  clear_error();
  const char *who = "mxa_assoc_score_firth";
  const char *bad = assoc_score_firth_args(plink, snps, indiv, P, ldp, R, ldr, Wt, ldw, H, ldh, n, kh, z_cutoff, penalty, tol, max_iter, score, var, zstat, beta, ldo);
  if (bad) { set_error(1, "%s: %s", who, bad); return 1; }
  bool out_dev = false;
  if (results_on_one_side(who, "score, var, zstat, beta, se, chisq and pval", {score, var, zstat, beta, se, chisq, pval}, &out_dev)) return 1;
  if (flag && (ptr_location(flag, nullptr) == 1) != out_dev) { set_error(1, "%s: flag and beta must be both host or both device pointers", who); return 1; }
  SpaArgs fit = {P, ldp, z_cutoff, tol, max_iter, pval, flag, ldo};
  fit.penalty = penalty;
  fit.beta = beta;
  fit.se = se;
  fit.chisq = chisq;
  return score_then_stage(who, plink, snps, indiv, R, ldr, Wt, ldw, H, ldh, n, kh, score, var, zstat, ldo, nobs, out_dev, fit);
}
