// mxa_assoc_set.hip -- set-based association (include/miraculix_amd.h: mxa_assoc_set, mxa_assoc_skat_pvalue): burden and SKAT statistics of
// SNP sets after the score scan of mxa_assoc_score.  The scan runs unchanged (mxa_assoc.hip: assoc_score_then); this unit is the stage that follows it on the
// scan's stream, as mxa_assoc_spa.hip is for the saddlepoint correction and the fit (the interface and what the kernels share: mxa_assoc_stage.h).  Per batch of sets: the rows of the batch's SNPs are gathered (a host matrix: into a bounce buffer; a device matrix is read in place),
// k_assoc_set_gram forms the weighted Gram S = X diag(w) X^T of every (set, trait) tile by tile on the fp64 MFMA, split over the individuals into pieces of
// kSetSplit, k_assoc_set_phi folds the pieces in ascending order, subtracts the covariate term and mirrors, k_assoc_set_stat and k_assoc_set_fold sum the six
// statistics.  No atomics anywhere: every sum over individuals runs in an order fixed by indiv alone, every sum over a set in an order fixed by its size alone,
// and no (set, trait) reads what another one wrote -- so a set's results do not depend on the batch it falls into or on the other sets of the call.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <vector>
#include "../../include/miraculix_amd.h"
#include "mxa_internal.h"
#include "mxa_assoc_set_host.h"
#include "mxa_assoc_stage.h"
#include "mxa_xprod.h"

namespace mxa {

namespace {

typedef double set_v4 __attribute__((ext_vector_type(4)));

struct SetDesc { int ent0, m, tj, tjp, c, pad; long s_off; };   // one (set, trait, tile pair tj <= tjp): the set's first entry in the batch, its size, the block of S
struct SetItem { int ent0, m, c, set; long s_off, t_off; };     // one (set, trait): ... and its first slot of the per-tile partial statistics

// ---- the hot path.  Workgroup blk0 + blockIdx.x = (work item, piece): the 16 x 16 tile (tj, tjp) of S of one (set, trait) over the individuals of piece p,
// [kSetSplit p, kSetSplit p + kSetSplit).  Wave v takes the logical words 64 p + v, + 4, ... of the piece (the words of assoc_load_word: the same fields for
// every alignment of a row).  Lane (r, g) = (lane & 15, lane >> 4) loads the word of row r of the A tile and of row r of the B tile (the diagonal tile: one
// load) and issues 16 v_mfma_f64_16x16x4_f64 a word: MFMA q takes the individuals 64 word + 4 q + g, A operand x (0, mu, 1, 2), B operand w x with the trait's
// working weight w, zero at and beyond indiv whatever the padding fields hold.  Rows at and beyond the set's size are zero words.  The four waves' tiles are
// added through the LDS as (w0 + w1) + (w2 + w3); slot t = 64 reg + lane of the partial is the element (row (lane >> 4) + 4 reg of tj, row lane & 15 of tjp).
__global__ void __launch_bounds__(256) k_assoc_set_gram(const uint8_t *__restrict__ rows, long bps, long indiv, const double *__restrict__ W,
                                                         const int *__restrict__ nobs, const int *__restrict__ c1, const int *__restrict__ c2,
                                                         const int *__restrict__ ent_snp, const int *__restrict__ ent_row, const SetDesc *__restrict__ desc,
                                                         long pieces, double *__restrict__ part, long blk0) {
  __shared__ double red[4][256];
  const long b = blk0 + blockIdx.x;
  const long di = b / pieces, p = b % pieces;
  const SetDesc d = desc[di];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const bool diag = d.tj == d.tjp;
  const int ja = kSetTile * d.tj + r, jb = kSetTile * d.tjp + r;
  const bool va = ja < d.m, vb = jb < d.m;
  double mu_a = 0.0, mu_b = 0.0;
  const uint8_t *row_a = rows, *row_b = rows;
  if (va) { mu_a = assoc_mu(nobs, c1, c2, ent_snp[d.ent0 + ja]); row_a = rows + (size_t)ent_row[d.ent0 + ja] * (size_t)bps; }
  if (vb) { mu_b = assoc_mu(nobs, c1, c2, ent_snp[d.ent0 + jb]); row_b = rows + (size_t)ent_row[d.ent0 + jb] * (size_t)bps; }
  const int sh_a = (int)(reinterpret_cast<uintptr_t>(row_a) & 15), sh_b = (int)(reinterpret_cast<uintptr_t>(row_b) & 15);
  const double *w = W + (size_t)d.c * (size_t)indiv;
  const long nwords = (bps + 15) / 16, words_per_piece = kSetSplit / 64;
  const long w_end = nwords < (p + 1) * words_per_piece ? nwords : (p + 1) * words_per_piece;
  set_v4 acc = {0.0, 0.0, 0.0, 0.0};
  for (long wd = p * words_per_piece + wave; wd < w_end; wd += 4) {
    AssocWord a = {0ull, 0ull}, bw = {0ull, 0ull};
    if (va) a = assoc_load_word(row_a, wd, bps, sh_a);
    if (diag) bw = a;
    else if (vb) bw = assoc_load_word(row_b, wd, bps, sh_b);
    const long i0 = 64 * wd + g;
    double wt[16];
#pragma unroll
    for (int q = 0; q < 16; q++) wt[q] = i0 + 4 * q < indiv ? w[i0 + 4 * q] : 0.0;
    const unsigned long long a_lo = a.lo >> (2 * g), a_hi = a.hi >> (2 * g), b_lo = bw.lo >> (2 * g), b_hi = bw.hi >> (2 * g);
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const unsigned ca = (unsigned)((q < 8 ? a_lo : a_hi) >> (8 * (q & 7))) & 3u, cb = (unsigned)((q < 8 ? b_lo : b_hi) >> (8 * (q & 7))) & 3u;
      const double xa = assoc_decode(ca, mu_a), xb = __dmul_rn(wt[q], assoc_decode(cb, mu_b));
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa, xb, acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int v = 0; v < 4; v++) red[wave][64 * v + lane] = acc[v];
  __syncthreads();
  const int t = threadIdx.x;
  part[((size_t)di * (size_t)pieces + (size_t)p) * 256 + (size_t)t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}

// ---- Phi from S and a, mirrored: workgroup blk0 + blockIdx.x = one work item of k_assoc_set_gram, thread t = its slot.  S = the pieces in ascending order;
// then, for the elements j <= j' inside the set, Phi = fma(-a_jh, a_j'h, Phi) over ascending h with a = fma(mu, M, D) as the scan's epilogue forms it; the
// one value goes to (j, j') and (j', j).
__global__ void __launch_bounds__(256) k_assoc_set_phi(const SetDesc *__restrict__ desc, long pieces, const double *__restrict__ part, const int *__restrict__ ent_snp,
                                                        const int *__restrict__ nobs, const int *__restrict__ c1, const int *__restrict__ c2,
                                                        const double *__restrict__ D, const double *__restrict__ M, long snps, int n, int kh,
                                                        double *__restrict__ phi, long blk0) {
  const long di = blk0 + blockIdx.x;
  const SetDesc d = desc[di];
  const int t = threadIdx.x;
  const int j = kSetTile * d.tj + ((t & 63) >> 4) + 4 * (t >> 6), jp = kSetTile * d.tjp + (t & 15);
  if (j >= d.m || jp >= d.m || j > jp) return;
  double v = 0.0;
  for (long p = 0; p < pieces; p++) v += part[((size_t)di * (size_t)pieces + (size_t)p) * 256 + (size_t)t];
  const long s = ent_snp[d.ent0 + j], sp = ent_snp[d.ent0 + jp];
  const double mu = assoc_mu(nobs, c1, c2, s), mup = assoc_mu(nobs, c1, c2, sp);
  for (int h = 0; h < kh; h++) {
    const size_t col = ((size_t)2 * (size_t)n + (size_t)d.c * (size_t)kh + (size_t)h) * (size_t)snps;
    const double a = __fma_rn(mu, M[col + (size_t)s], D[col + (size_t)s]), ap = __fma_rn(mup, M[col + (size_t)sp], D[col + (size_t)sp]);
    v = __fma_rn(-a, ap, v);
  }
  double *o = phi + d.s_off;
  o[(size_t)j + (size_t)jp * (size_t)d.m] = v;
  o[(size_t)jp + (size_t)j * (size_t)d.m] = v;
}

// ---- the sums over pairs: workgroup blk0 + blockIdx.x = slot of (item, row tile rb) takes the rows j in [16 rb, 16 rb + 16) of A = diag(omega) Phi
// diag(omega), A_jj' = (omega_j Phi_jj') omega_j'.  Thread t takes the columns j' = t, t + 256, ... in ascending order and, per column, the tile's rows in
// ascending order: varB += A_jj', c2 = fma(A_jj', A_jj', c2), and (A A)_jj' = the chain fma(A_jl, A_lj', .) over ascending l, never stored,
// c4 = fma((A A)_jj', (A A)_jj', c4).  The three sums of the slot end in assoc_block_sums; k_assoc_set_fold adds the slots of an item in ascending order.
__global__ void __launch_bounds__(256) k_assoc_set_stat(const SetItem *__restrict__ items, const int *__restrict__ tile_item, const double *__restrict__ ent_wt,
                                                         const double *__restrict__ phi, double *__restrict__ spart, long blk0) {
  __shared__ double red[3][4];
  const long slot = blk0 + blockIdx.x;
  const SetItem it = items[tile_item[slot]];
  const int m = it.m, j0 = kSetTile * (int)(slot - it.t_off);
  const double *P = phi + it.s_off, *om = ent_wt + it.ent0;
  double v[3] = {0.0, 0.0, 0.0};
  for (int jp = threadIdx.x; jp < m; jp += 256) {
    const double wp = om[jp];
    const double *colp = P + (size_t)jp * (size_t)m;
    for (int j = j0; j < j0 + kSetTile && j < m; j++) {
      const double wj = om[j];
      const double *colj = P + (size_t)j * (size_t)m;      // Phi_jl = Phi_lj bit for bit: row j is read as column j
      const double A = __dmul_rn(__dmul_rn(wj, colp[j]), wp);
      v[0] += A;
      v[1] = __fma_rn(A, A, v[1]);
      double aa = 0.0;
      for (int l = 0; l < m; l++) {
        const double wl = om[l];
        aa = __fma_rn(__dmul_rn(__dmul_rn(wj, colj[l]), wl), __dmul_rn(__dmul_rn(wl, colp[l]), wp), aa);
      }
      v[2] = __fma_rn(aa, aa, v[2]);
    }
  }
  assoc_block_sums<3>(v, red);
  if (threadIdx.x < 3) spart[3 * (size_t)slot + threadIdx.x] = v[threadIdx.x];
}

// ---- one thread per (set, trait) of the batch: B, Q and c1 over the set's entries in ascending order, varB, c2 and c4 over its slots in ascending order
__global__ void __launch_bounds__(256) k_assoc_set_fold(long nitems, const SetItem *__restrict__ items, const int *__restrict__ ent_snp,
                                                         const double *__restrict__ ent_wt, const double *__restrict__ U, long ldu, const double *__restrict__ phi,
                                                         const double *__restrict__ spart, double *__restrict__ stat, long lds, long blk0) {
  const long i = (blk0 + blockIdx.x) * 256 + threadIdx.x;
  if (i >= nitems) return;
  const SetItem it = items[i];
  const double *P = phi + it.s_off;
  double B = 0.0, Q = 0.0, t1 = 0.0, vB = 0.0, t2 = 0.0, t4 = 0.0;
  for (int j = 0; j < it.m; j++) {
    const double om = ent_wt[it.ent0 + j];
    const double u = __dmul_rn(om, U[(size_t)ent_snp[it.ent0 + j] + (size_t)it.c * (size_t)ldu]);
    B += u;
    Q = __fma_rn(u, u, Q);
    t1 += __dmul_rn(__dmul_rn(om, P[(size_t)j * (size_t)it.m + (size_t)j]), om);
  }
  const long tiles = (it.m + kSetTile - 1) / kSetTile;
  for (long rb = 0; rb < tiles; rb++) {
    const double *sp = spart + 3 * (size_t)(it.t_off + rb);
    vB += sp[0]; t2 += sp[1]; t4 += sp[2];
  }
  double *o = stat + (size_t)it.set + (size_t)6 * (size_t)it.c * (size_t)lds;
  o[0] = B; o[(size_t)lds] = vB; o[2 * (size_t)lds] = Q; o[3 * (size_t)lds] = t1; o[4 * (size_t)lds] = t2; o[5 * (size_t)lds] = t4;
}

// ---- host side
struct SetBatchHost {                 // what one batch uploads; alive until the stage's last wait
  std::vector<int> ent_snp, ent_row, tile_item;
  std::vector<double> ent_wt;
  std::vector<SetDesc> desc;
  std::vector<SetItem> items;
  std::vector<int> rows;              // a host matrix: the batch's distinct SNPs, ascending = the rows of the bounce buffer
};

struct SetStage {
  int nsets, n;
  const long *set_ptr;
  const int *set_idx;
  const double *set_wt;
  double *stat, *phi;
  long lds;
  bool in_place;
  std::vector<SetBatch> plan;
  std::vector<SetBatchHost> host;
  size_t max_ent = 0, max_desc = 0, max_items = 0, max_tiles = 0, max_phi = 0;   // per buffer, over the batches: each may come from another batch
  long max_rows = 0;

  void prepare() {
    host.resize(plan.size());
    for (size_t bi = 0; bi < plan.size(); bi++) {
      const SetBatch &b = plan[bi];
      SetBatchHost &h = host[bi];
      const long e0 = set_ptr[b.k0];
      h.ent_snp.assign(set_idx + e0, set_idx + e0 + b.entries);
      h.ent_wt.assign((size_t)b.entries, 1.0);
      if (set_wt) h.ent_wt.assign(set_wt + e0, set_wt + e0 + b.entries);
      if (in_place) h.ent_row = h.ent_snp;
      else {
        h.rows = h.ent_snp;
        std::sort(h.rows.begin(), h.rows.end());
        h.rows.erase(std::unique(h.rows.begin(), h.rows.end()), h.rows.end());
        h.ent_row.resize(h.ent_snp.size());
        for (size_t e = 0; e < h.ent_snp.size(); e++) h.ent_row[e] = (int)(std::lower_bound(h.rows.begin(), h.rows.end(), h.ent_snp[e]) - h.rows.begin());
      }
      long s_off = 0, t_off = 0;
      for (int k = b.k0; k < b.k1; k++) {
        const int m = (int)(set_ptr[k + 1] - set_ptr[k]), ent0 = (int)(set_ptr[k] - e0);
        const int tiles = (int)set_tiles(m);
        for (int c = 0; c < n; c++) {
          const int item = (int)h.items.size();
          h.items.push_back({ent0, m, c, k, s_off, t_off});
          for (int tj = 0; tj < tiles; tj++)
            for (int tjp = tj; tjp < tiles; tjp++) h.desc.push_back({ent0, m, tj, tjp, c, 0, s_off});
          for (int rb = 0; rb < tiles; rb++) h.tile_item.push_back(item);
          s_off += (long)m * m;
          t_off += tiles;
        }
      }
      max_ent = std::max(max_ent, (size_t)b.entries); max_desc = std::max(max_desc, (size_t)b.descs); max_items = std::max(max_items, (size_t)b.items);
      max_tiles = std::max(max_tiles, (size_t)b.tiles); max_phi = std::max(max_phi, b.phi_doubles);
      max_rows = std::max(max_rows, (long)h.rows.size());
    }
  }
  // device memory of the stage, buffer by buffer as run() allocates them (each sized by its largest batch): the bounce rows, S / Phi, the partial sums of
  // 2 KiB per (set, trait, tile pair, piece), the per-tile sums, the lists of a batch, the device copy of a host stat
  size_t bytes(long indiv, long bps, bool out_dev) const {
    return sizeof(double) * (max_phi + max_desc * (size_t)set_pieces(indiv) * 256 + 3 * max_tiles) + max_ent * (2 * sizeof(int) + sizeof(double)) +
           max_desc * sizeof(SetDesc) + max_items * sizeof(SetItem) + max_tiles * sizeof(int) + (size_t)max_rows * (size_t)bps +
           (out_dev ? 0 : sizeof(double) * (size_t)nsets * 6 * (size_t)n) + 4096;
  }

  int run(const AssocScanView &v, const unsigned char *plink) {
    hipStream_t s = v.s;
    const long pieces = set_pieces(v.indiv);
    XBuf bSnp, bRow, bWt, bDesc, bItems, bTileItem, bPhi, bPart, bSpart, bStat, bRows;
    if (bSnp.alloc(sizeof(int) * max_ent) || bRow.alloc(sizeof(int) * max_ent) || bWt.alloc(sizeof(double) * max_ent) || bDesc.alloc(sizeof(SetDesc) * max_desc) ||
        bItems.alloc(sizeof(SetItem) * max_items) || bTileItem.alloc(sizeof(int) * max_tiles) || bPhi.alloc(sizeof(double) * max_phi) ||
        bPart.alloc(sizeof(double) * max_desc * (size_t)pieces * 256) || bSpart.alloc(sizeof(double) * 3 * max_tiles) ||
        (!in_place && bRows.alloc((size_t)max_rows * (size_t)v.bps)))
      return 1;
    double *d_stat = stat;
    long ld_stat = lds;
    if (!v.out_dev) { if (bStat.alloc(sizeof(double) * (size_t)nsets * 6 * (size_t)n)) return 1; d_stat = (double *)bStat.p; ld_stat = nsets; }
    size_t phi_done = 0;
    for (size_t bi = 0; bi < plan.size(); bi++) {
      const SetBatch &b = plan[bi];
      const SetBatchHost &h = host[bi];
      if (b.entries > 0) {
        MXA_HIP(hipMemcpyAsync(bSnp.p, h.ent_snp.data(), sizeof(int) * (size_t)b.entries, hipMemcpyHostToDevice, s));
        MXA_HIP(hipMemcpyAsync(bRow.p, h.ent_row.data(), sizeof(int) * (size_t)b.entries, hipMemcpyHostToDevice, s));
        MXA_HIP(hipMemcpyAsync(bWt.p, h.ent_wt.data(), sizeof(double) * (size_t)b.entries, hipMemcpyHostToDevice, s));
      }
      if (b.descs > 0) {
        MXA_HIP(hipMemcpyAsync(bDesc.p, h.desc.data(), sizeof(SetDesc) * (size_t)b.descs, hipMemcpyHostToDevice, s));
        MXA_HIP(hipMemcpyAsync(bTileItem.p, h.tile_item.data(), sizeof(int) * (size_t)b.tiles, hipMemcpyHostToDevice, s));
      }
      MXA_HIP(hipMemcpyAsync(bItems.p, h.items.data(), sizeof(SetItem) * (size_t)b.items, hipMemcpyHostToDevice, s));
      const uint8_t *d_rows = plink;
      if (!in_place) {                          // the batch's distinct rows of a host matrix into the bounce buffer
        if (assoc_gather_rows((uint8_t *)bRows.p, plink, v.bps, h.rows.data(), (long)h.rows.size(), s)) return 1;
        d_rows = (const uint8_t *)bRows.p;
      }
      if (b.descs > 0) {
        launch_in_block_chunks(b.descs * pieces, [&](unsigned nb, long b0) {
          k_assoc_set_gram<<<nb, 256, 0, s>>>(d_rows, v.bps, v.indiv, v.W, v.nobs, v.c1, v.c2, (const int *)bSnp.p, (const int *)bRow.p, (const SetDesc *)bDesc.p, pieces,
                                              (double *)bPart.p, b0);
        });
        launch_in_block_chunks(b.descs, [&](unsigned nb, long b0) {
          k_assoc_set_phi<<<nb, 256, 0, s>>>((const SetDesc *)bDesc.p, pieces, (const double *)bPart.p, (const int *)bSnp.p, v.nobs, v.c1, v.c2, v.D, v.M, v.snps, v.n,
                                             v.kh, (double *)bPhi.p, b0);
        });
        launch_in_block_chunks(b.tiles, [&](unsigned nb, long b0) {
          k_assoc_set_stat<<<nb, 256, 0, s>>>((const SetItem *)bItems.p, (const int *)bTileItem.p, (const double *)bWt.p, (const double *)bPhi.p, (double *)bSpart.p, b0);
        });
      }
      launch_in_block_chunks((b.items + 255) / 256, [&](unsigned nb, long b0) {
        k_assoc_set_fold<<<nb, 256, 0, s>>>(b.items, (const SetItem *)bItems.p, (const int *)bSnp.p, (const double *)bWt.p, v.U, v.ldu, (const double *)bPhi.p,
                                            (const double *)bSpart.p, d_stat, ld_stat, b0);
      });
      MXA_HIP(hipGetLastError());
      if (phi && b.phi_doubles > 0) MXA_HIP(hipMemcpyAsync(phi + phi_done, bPhi.p, sizeof(double) * b.phi_doubles, hipMemcpyDefault, s));
      phi_done += b.phi_doubles;
    }
    if (!v.out_dev) {
      const size_t col = sizeof(double) * (size_t)nsets;
      MXA_HIP(hipMemcpy2DAsync(stat, sizeof(double) * (size_t)lds, d_stat, col, col, (size_t)6 * (size_t)n, hipMemcpyDeviceToHost, s));
    }
    MXA_HIP(hipStreamSynchronize(s));           // the buffers of the stage are released on return
    return 0;
  }
};

int set_stage_run(void *self, const AssocScanView &v, const unsigned char *plink) { return static_cast<SetStage *>(self)->run(v, plink); }

}  // namespace

}  // namespace mxa

extern "C" int mxa_assoc_set(const unsigned char *plink, int snps, int indiv, const double *R, long ldr, const double *Wt, long ldw, const double *H, long ldh, int n,
                             int kh, int nsets, const long *set_ptr, const int *set_idx, const double *set_wt, double *score, double *var, double *zstat, long ldo,
                             int *nobs, double *stat, long lds, double *phi) {
  using namespace mxa;
  clear_error();
  const char *who = "mxa_assoc_set";
  char msg[192];
  if (assoc_set_args(plink, snps, indiv, R, ldr, Wt, ldw, H, ldh, n, kh, nsets, set_ptr, set_idx, score, var, zstat, ldo, stat, lds, msg, sizeof(msg))) {
    set_error(1, "%s: %s", who, msg);
    return 1;
  }
  bool out_dev = false;
  if (results_on_one_side(who, "score, var, zstat, stat and phi", {score, var, zstat, stat, phi}, &out_dev)) return 1;
  DeviceRestore restore;
  const int dev = select_device();
  if (dev < 0) return 1;
  SetStage st = {nsets, n, set_ptr, set_idx, set_wt, stat, phi, lds, assoc_rows_in_place(plink, dev)};
  long max_entries = LONG_MAX;
  const char *e = getenv("MXA_ASSOC_SET_BATCH");
  if (e && atol(e) > 0) max_entries = atol(e);
  st.plan = set_plan(nsets, set_ptr, n, indiv, max_entries, kSetBudget);
  st.prepare();
  const AssocAfterScan after = {who, st.bytes(indiv, ((long)indiv + 3) / 4, out_dev), {true, false, false}, &st, set_stage_run};   // the stage reads U alone
  return assoc_score_then(plink, snps, indiv, R, ldr, Wt, ldw, H, ldh, n, kh, score, var, zstat, ldo, nobs, out_dev, after);
}

extern "C" int mxa_assoc_skat_pvalue(long count, const double *Q, const double *c1, const double *c2, const double *c4, double *pval, double *df) {
  using namespace mxa;
  clear_error();
  const char *who = "mxa_assoc_skat_pvalue";
  if (count < 0) { set_error(1, "%s: count must not be negative", who); return 1; }
  if (count > 0 && (!Q || !c1 || !c2 || !c4 || !pval)) { set_error(1, "%s: Q, c1, c2, c4 and pval must not be NULL", who); return 1; }
  for (long i = 0; i < count; i++) pval[i] = skat_pvalue_host(Q[i], c1[i], c2[i], c4[i], df ? df + i : nullptr);
  return 0;
}
