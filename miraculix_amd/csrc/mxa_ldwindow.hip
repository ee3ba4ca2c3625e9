// mxa_ldwindow.hip -- windowed LD: the entries of mxa_ld's R inside a window, without the snps x snps matrix.  The fixed window (mxa_ld_band,
// mxa_ld_scores and their _pairwise forms) and the general one (mxa_ld_window_rows / _scores / _pairs / _apply, plain and _pairwise; mxa_ld_window_bounds).
// LdWindow is one call of an entry: checks, tile plan, pre-flight, buffers, finish.  Two routes stage the operand: the plain one runs the window's tiles
// through the crossproduct kernels' window epilogue (mxa_crossprod.hip), the pairwise-complete one and every pairs / apply entry run them into int32 count
// slots (kPostCounts) and read those back here -- LdCountRun is that pipeline, the providers are the value of one element.
#include "../../include/miraculix_amd.h"
#include "mxa_xprod.h"
#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <cstring>

namespace mxa {

// ---- windowed LD: the band |i - j| <= window of R, as LAPACK lower band storage (scores == 0: out = band, leading dimension ldb, flag = kind) or reduced to
// the LD scores (scores != 0: out = scores, flag = adjust).  O(snps * window) work and memory: the tiles of band_tiles through the same kernels as mxa_ld.
// zeros of the band's tail band[d + i * ldb], i + d >= n: window (window + 1) / 2 elements of the last `window` SNPs, not a pass over the band
__global__ void __launch_bounds__(256) k_ld_band_tail(double *__restrict__ band, long ldb, long n, long window) {
  const long i = n - 1 - (long)blockIdx.x;                    // blockIdx.x < window < n
  for (long d = n - i + threadIdx.x; d <= window; d += 256) band[(size_t)d + (size_t)i * ldb] = 0.0;
}
// scores[i] = the slots of row i in a fixed order: the I side of the tiles (I, I + dt), then the J side of the tiles (I - dt, I); a slot exists iff its tile
// does, and tile row I holds the tiles up to column jmax[I] (nb ints, non-decreasing)
__global__ void __launch_bounds__(256) k_ld_score_finish(const double *__restrict__ P, long n, long stride, const int *__restrict__ jmax, int ndiag, double *__restrict__ scores) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int I = (int)(i / kXT);
  double s = 0.0;
  for (int dt = 0; dt <= ndiag; dt++) if (I + dt <= jmax[I]) s += P[ld_score_slot(0, dt, ndiag, stride) + (size_t)i];
  for (int dt = 1; dt <= ndiag; dt++) if (I - dt >= 0 && jmax[I - dt] >= I) s += P[ld_score_slot(1, dt, ndiag, stride) + (size_t)i];
  scores[i] = s;
}

// a host result of the windowed entries: the scores or the ragged rows as they are, or the compact device band (leading dimension window + 1) into the
// caller's band of leading dimension ldb
static int ld_window_download(const double *d_res, size_t obytes, long snps, long window, double *out, long ldb, bool compact, hipStream_t s) {
  if (compact || ldb == window + 1) MXA_HIP(hipMemcpyAsync(out, d_res, obytes, hipMemcpyDeviceToHost, s));
  else {   // a wider host ldb: one download, then the rows d <= window of every column (the rows beyond stay the caller's)
    std::vector<double> h((size_t)(window + 1) * (size_t)snps);
    MXA_HIP(hipMemcpyAsync(h.data(), d_res, obytes, hipMemcpyDeviceToHost, s));
    MXA_HIP(hipStreamSynchronize(s));
    for (long i = 0; i < snps; i++) memcpy(out + (size_t)i * ldb, h.data() + (size_t)i * (window + 1), sizeof(double) * (size_t)(window + 1));
  }
  return 0;
}

namespace {
// One call of a windowed entry: everything around the route's own staging and tile launches.  begin(): the shared argument checks, the tile plan, the sizes,
// the pre-flight, the stream, the operand / result / partial buffers and the events; start() and finish() enclose the launches: d_dst (leading dimension
// ld_dst) is where they write -- the band, the rows, or the scores' partial buffer P -- and finish() turns it into the result at d_res and delivers that.
// Two ways of constructing it: the fixed window (`window` SNPs on each side; result = band of leading dimension ldb, or scores) and the general one
// (last != nullptr: the window of SNP i ends at last[i]; result = ragged rows, or scores).  Both end in the same plan, jmax[] per tile row.
// Two more results of the general window.  set_pairs(): the pairs above a cutoff as CSR (mxa_ld_window_pairs*); `out` is then the caller's rowptr, and a host
// result leaves from one device buffer d_out = rowptr (snps + 1 longs), val (capacity doubles), col (capacity ints).  set_apply(): the window applied to a
// matrix (mxa_ld_window_apply*); out = Y, ldb = ldy, the result is snps x ncols.
enum class LdResult { kRows, kScores, kPairsCount, kPairsFill, kApply };   // kRows: the band (fixed window) or the ragged rows; kPairsFill: col / val are written
struct LdWindow {
  const char *who;
  const unsigned char *plink;
  long snps, indiv, window;
  const int *last;             // the caller's, host or device; nullptr: the fixed window
  double *out;
  long ldb;
  LdResult result;
  int flag;                    // kind (band, rows, pairs) / adjust (scores)
  int *col = nullptr;
  double *val = nullptr;
  long capacity = 0;           // entries of col / val (0 on a count-only call)
  long *total = nullptr;       // the CSR result: where the number of pairs goes
  int ncols = 0;
  XGeom g;
  long row_bytes = 0;
  int ndiag = 0;               // tile diagonals of the partial buffer: the kernels' (ld_band_diagonals(window)), or max(jmax[I] - I)
  std::vector<int> jmax;       // tile row I holds the tiles (I, I .. jmax[I])
  size_t ntiles = 0, row_tiles_max = 0;
  bool in_dev = false, out_dev = false;
  size_t plane_bytes = 0, obytes = 0;
  XStream st;
  hipStream_t s = nullptr;
  XBuf d_X, bounce, d_out, d_flag, d_P, d_jmax, d_last, d_rowptr;
  XEvent e0, e1;
  double *d_res = nullptr, *d_dst = nullptr;
  long ld_res = 0, ld_dst = 0;
  LdWindow(const char *who_, const unsigned char *plink_, long snps_, long indiv_, long window_, const int *last_, double *out_, long ldb_, bool scores_, int flag_)
      : who(who_), plink(plink_), snps(snps_), indiv(indiv_), window(window_), last(last_), out(out_), ldb(ldb_), result(scores_ ? LdResult::kScores : LdResult::kRows),
        flag(flag_), g(indiv_, snps_) {}
  bool scores() const { return result == LdResult::kScores; }
  bool pairs() const { return result == LdResult::kPairsCount || result == LdResult::kPairsFill; }
  const uint8_t *X() const { return (const uint8_t *)d_X.p; }
  bool general() const { return last != nullptr; }
  // the epilogue kind of the crossproduct kernels and what they take for `c0`
  int post_kind() const { return scores() ? kPostLdScores : kPostLdBand; }
  long post_c0() const { return general() ? (long)ndiag : window; }
  void set_post(XPost &xp) const { xp.do_scale = flag; xp.last = (const int *)d_last.p; xp.rowptr = (const long *)d_rowptr.p; }
  std::vector<int4> tiles() const { return window_tiles(jmax); }
  void set_apply(int ncols_) { result = LdResult::kApply; ncols = ncols_; }
  void set_pairs(int *col_, double *val_, long capacity_, long *total_) {
    result = col_ ? LdResult::kPairsFill : LdResult::kPairsCount;
    col = col_; val = val_; capacity = col_ ? capacity_ : 0; total = total_;
  }
  // where the CSR result is formed on the device: the caller's arrays, or the pieces of d_out
  long *d_pairs_rowptr() const { return out_dev ? reinterpret_cast<long *>(out) : (long *)d_out.p; }
  double *d_pairs_val() const { return out_dev ? val : reinterpret_cast<double *>((long *)d_out.p + snps + 1); }
  int *d_pairs_col() const { return out_dev ? col : reinterpret_cast<int *>(d_pairs_val() + capacity); }

  // The tile plan.  Fixed: the band of ndiag tile diagonals.  General: `last` is fetched (host or device pointer) and checked, rowptr formed, and tile row I
  // reaches as far as its last SNP does (last is non-decreasing), so every tile (I, I .. jmax[I]) holds a window element.
  int plan(std::vector<long> &h_rowptr, std::vector<int> &h_last) {
    jmax.resize((size_t)g.nb);
    if (!general()) {
      ndiag = ld_band_diagonals(window);
      for (int I = 0; I < g.nb; I++) jmax[(size_t)I] = std::min(g.nb - 1, I + ndiag);
    } else {
      h_last.resize((size_t)snps);
      MXA_HIP(hipMemcpy(h_last.data(), last, sizeof(int) * (size_t)snps, hipMemcpyDefault));
      h_rowptr.resize((size_t)snps + 1);
      h_rowptr[0] = 0;
      for (long i = 0; i < snps; i++) {
        const long l = h_last[(size_t)i];
        if (l < i || l >= snps || (i > 0 && l < h_last[(size_t)i - 1])) {
          set_error(1, "%s: need i <= last[i] < snps, non-decreasing (last[%ld] = %ld, snps %ld)", who, i, l, snps);
          return 1;
        }
        h_rowptr[(size_t)i + 1] = h_rowptr[(size_t)i] + (l - i + 1);
      }
      ndiag = 0;
      for (int I = 0; I < g.nb; I++) {
        jmax[(size_t)I] = h_last[(size_t)std::min<long>((long)I * kXT + kXT - 1, snps - 1)] / kXT;
        ndiag = std::max(ndiag, jmax[(size_t)I] - I);
      }
    }
    for (int I = 0; I < g.nb; I++) {
      const size_t t = (size_t)(jmax[(size_t)I] - I + 1);
      ntiles += t;
      row_tiles_max = std::max(row_tiles_max, t);
    }
    return 0;
  }

  // planes: of the staged operand; extra_bytes(): what the route allocates beyond the operand, the result and the partial buffer, for the pre-flight (called
  // once the plan stands).  The checks run in the order in which the entries have always reported them, so the two that only one route has are passed in:
  // route_error (a complete message, or nullptr) is reported behind "bad arguments", max_indiv (0: no bound) in front of the SNP bound; adj_msg, snps_msg:
  // the route's wording.
  template <typename Extra>
  int begin(int planes, Extra extra_bytes, const char *route_error, long max_indiv, const char *adj_msg, const char *snps_msg) {
    if (!plink || !out || snps <= 0 || indiv <= 0) { set_error(1, "%s: bad arguments", who); return 1; }
    if (route_error) { set_error(1, route_error, who); return 1; }
    if (!general() && (window < 0 || window >= snps)) { set_error(1, "%s: need 0 <= window < snps (window %ld, snps %ld)", who, window, snps); return 1; }
    if (flag != 0 && flag != 1) { set_error(1, "%s: %s must be 0 or 1", who, scores() ? "adjust" : "kind"); return 1; }
    if (!general() && !scores() && ldb < window + 1) { set_error(1, "%s: need ldb >= window + 1 (ldb %ld, window %ld)", who, ldb, window); return 1; }
    if (scores() && flag && indiv < 3) { set_error(1, adj_msg, who); return 1; }
    if (max_indiv && indiv > max_indiv) { set_error(1, "%s: at most %ld individuals per call (4 indiv^2 must stay below 2^53)", who, max_indiv); return 1; }
    if (snps >= kXFusedMaxRows) { set_error(1, snps_msg, who, kXFusedMaxRows - 1); return 1; }
    if (select_device() < 0) return 1;
    std::vector<long> h_rowptr;
    std::vector<int> h_last;
    if (plan(h_rowptr, h_last)) return 1;
    row_bytes = (indiv + 3) / 4;
    in_dev = ptr_location(plink, nullptr) == 1;
    out_dev = ptr_location(out, nullptr) == 1;
    if (result == LdResult::kPairsFill && ((ptr_location(col, nullptr) == 1) != out_dev || (val && (ptr_location(val, nullptr) == 1) != out_dev))) {   // val == nullptr: the library's own "no val" fill
      set_error(1, "%s: rowptr, col and val must be all host or all device pointers", who);
      return 1;
    }
    // a host band leaves from a compact device copy (leading dimension window + 1); the scores' partial buffer holds 2 (ndiag + 1) slots per SNP
    plane_bytes = (size_t)g.rows_pad() * g.pitch();
    switch (result) {
      case LdResult::kRows: obytes = sizeof(double) * (general() ? (size_t)h_rowptr.back() : (size_t)(window + 1) * (size_t)snps); break;
      case LdResult::kScores: obytes = sizeof(double) * (size_t)snps; break;
      case LdResult::kPairsCount:
      case LdResult::kPairsFill: obytes = sizeof(long) * ((size_t)snps + 1) + (sizeof(double) + sizeof(int)) * (size_t)capacity; break;
      case LdResult::kApply: obytes = sizeof(double) * (size_t)snps * (size_t)ncols; break;   // a host Y leaves from a compact device copy (leading dimension snps)
    }
    const size_t pbytes = scores() ? sizeof(double) * ld_score_slot(2, 0, ndiag, g.rows_pad()) : 0;
    const size_t wbytes = sizeof(int) * (size_t)g.nb + (general() ? sizeof(int) * (size_t)snps + sizeof(long) * ((size_t)snps + 1) : 0);   // jmax, last, rowptr
    size_t free_b = 0, total_b = 0;
    MXA_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t need = planes * plane_bytes + pbytes + wbytes + extra_bytes() + (out_dev ? 0 : obytes) + (in_dev ? 0 : (size_t)stage_chunk_rows(snps, (size_t)row_bytes, (size_t)256 << 20) * row_bytes);   // the bounce buffer stage_operand allocates
    if (need > free_b) { set_error(12, "%s: not enough device memory: required %zu GB, free %zu GB", who, need >> 30, free_b >> 30); return 1; }
    if (st.create(hipStreamDefault)) return 1;   // blocking: ordered against the caller's default-stream work
    s = st.s;
    if (d_X.alloc(planes * plane_bytes) || d_flag.alloc(sizeof(int)) || (!out_dev && d_out.alloc(obytes)) || (scores() && d_P.alloc(pbytes))) return 1;
    // the plan's arrays: synchronous copies (the host vectors end with this function)
    if (scores()) {
      if (d_jmax.alloc(sizeof(int) * (size_t)g.nb)) return 1;
      MXA_HIP(hipMemcpy(d_jmax.p, jmax.data(), sizeof(int) * (size_t)g.nb, hipMemcpyHostToDevice));
    }
    if (general()) {
      const bool rows = result == LdResult::kRows;   // the ragged rows' starts
      if (d_last.alloc(sizeof(int) * (size_t)snps) || (rows && d_rowptr.alloc(sizeof(long) * ((size_t)snps + 1)))) return 1;
      MXA_HIP(hipMemcpy(d_last.p, h_last.data(), sizeof(int) * (size_t)snps, hipMemcpyHostToDevice));
      if (rows) MXA_HIP(hipMemcpy(d_rowptr.p, h_rowptr.data(), sizeof(long) * ((size_t)snps + 1), hipMemcpyHostToDevice));
    }
    d_res = out_dev ? out : (double *)d_out.p;
    ld_res = out_dev ? ldb : window + 1;
    d_dst = scores() ? (double *)d_P.p : d_res;
    ld_dst = scores() ? g.rows_pad() : ld_res;
    return e0.create() || e1.create();
  }
  int start() { MXA_HIP(hipEventRecord(e0.e, s)); return 0; }
  // The last launches of the result kind, the second event, the result's way to a host caller, and the stream's end: the lifetime of the route's tile lists,
  // statistics, scratch and partials.  d_total (the CSR result): the running base after the last group.
  int finish(const long *d_total = nullptr) {
    if (scores()) hipLaunchKernelGGL(k_ld_score_finish, dim3((unsigned)((snps + 255) / 256)), dim3(256), 0, s, (const double *)d_P.p, snps, g.rows_pad(), (const int *)d_jmax.p, ndiag, d_res);
    else if (result == LdResult::kRows && !general() && window > 0) hipLaunchKernelGGL(k_ld_band_tail, dim3((unsigned)window), dim3(256), 0, s, d_res, ld_res, snps, window);
    MXA_HIP(hipGetLastError());
    MXA_HIP(hipEventRecord(e1.e, s));
    long h_total = 0;
    if (pairs()) MXA_HIP(hipMemcpyAsync(&h_total, d_total, sizeof(long), hipMemcpyDeviceToHost, s));   // read once
    if (!out_dev) {   // a host result: rowptr now and col / val below; Y's snps rows of every column from the compact device copy; the scores, rows or band
      if (pairs()) MXA_HIP(hipMemcpyAsync(out, d_pairs_rowptr(), sizeof(long) * ((size_t)snps + 1), hipMemcpyDeviceToHost, s));
      else if (result == LdResult::kApply) MXA_HIP(hipMemcpy2DAsync(out, sizeof(double) * (size_t)ldb, d_res, sizeof(double) * (size_t)snps, sizeof(double) * (size_t)snps, (size_t)ncols, hipMemcpyDeviceToHost, s));
      else if (ld_window_download(d_res, obytes, snps, window, out, ldb, scores() || general(), s)) return 1;
    }
    MXA_HIP(hipStreamSynchronize(s));
    const size_t filled = pairs() ? (size_t)std::min(h_total, capacity) : 0;   // the first min(total, capacity) entries of col / val
    if (!out_dev && filled) {
      MXA_HIP(hipMemcpyAsync(val, d_pairs_val(), sizeof(double) * filled, hipMemcpyDeviceToHost, s));
      MXA_HIP(hipMemcpyAsync(col, d_pairs_col(), sizeof(int) * filled, hipMemcpyDeviceToHost, s));
      MXA_HIP(hipStreamSynchronize(s));
    }
    MXA_HIP(profile_launch(e0, e1));
    if (!pairs()) return 0;
    *total = h_total;
    // total > capacity: error 25, rowptr and *total valid
    if (result == LdResult::kPairsFill && h_total > capacity) { set_error(25, "%s: %ld pairs pass the cutoff, capacity is %ld", who, h_total, capacity); return 1; }
    return 0;
  }
};
}  // namespace

// the operand of the plain route: staged as it is, the engine, the frequencies on the device and the LD map's statistics (xp.u, xp.w, xp.a)
namespace {
struct LdPlainOperand {
  bool f4 = false;
  XBuf f_tmp, stats[3];
  XPost xp;
  int stage(LdWindow &c, const unsigned char *plink, bool is_plink, const double *freq) {
    hipStream_t s = c.s;
    if (stage_operand(plink, c.in_dev, c.row_bytes, is_plink, c.g, (uint8_t *)c.d_X.p, (int *)c.d_flag.p, c.bounce, s, 0, c.indiv)) return 1;   // padding bits are no individuals
    if (pick_engine((const int *)c.d_flag.p, c.indiv, s, f4)) return 1;
    const double *d_f = freq;
    if (ptr_location(freq, nullptr) != 1) {
      if (f_tmp.alloc(sizeof(double) * (size_t)c.snps)) return 1;
      MXA_HIP(hipMemcpyAsync(f_tmp.p, freq, sizeof(double) * (size_t)c.snps, hipMemcpyHostToDevice, s));
      d_f = (const double *)f_tmp.p;
    }
    return fused_post_stats(c.g, c.X(), c.indiv, kPostLd, 0, d_f, stats, s, xp);
  }
};
}  // namespace

// the plain route: the operand staged as it is, the LD map's statistics, and one launch of the window's tiles with the window epilogue
int ld_window_any(const char *who, const unsigned char *plink, long snps, long indiv, long window, const int *last, double *out, long ldb, bool scores, int flag,
                         bool is_plink, const double *freq) {
  LdWindow c(who, plink, snps, indiv, window, last, out, ldb, scores, flag);
  if (c.begin(1, [] { return (size_t)0; }, freq ? nullptr : "%s: allele frequencies are required", 0, "%s: the adjusted estimator r^2 - (1 - r^2) / (indiv - 2) needs indiv >= 3",
              "%s: at most %ld SNPs per call (the fused statistics)")) return 1;
  const XGeom &g = c.g;
  hipStream_t s = c.s;
  LdPlainOperand op;
  if (op.stage(c, plink, is_plink, freq)) return 1;
  XPost &xp = op.xp;
  c.set_post(xp);                                         // kind / adjust, the general window's arrays (xprod_store_window)
  XTiles t;
  if (upload_tiles({c.tiles()}, s, t)) return 1;
  if (c.start() || t.launch(0, g, op.f4, s, c.X(), c.d_dst, c.ld_dst, c.post_c0(), nullptr, c.post_kind(), xp)) return 1;
  return c.finish();
}

// ---- pairwise-complete windowed LD (mxa_ld_band_pairwise, mxa_ld_scores_pairwise): Pearson's r of SNPs i, j over the individuals genotyped at BOTH.
// With the planes Z, M, A of k_xstage_planes every ingredient is an exact integer crossproduct of rows:
//   N = M_i.M_j   Sxy = Z_i.Z_j   Sx = Z_i.M_j   Sy = M_i.Z_j   Sxx = Sx + 2 A_i.M_j   Syy = Sy + 2 M_i.A_j
//   num = N Sxy - Sx Sy   dx = N Sxx - Sx^2   dy = N Syy - Sy^2   r = num / sqrt(dx dy)
// Six tile products per band tile (count store into a scratch slot each), then k_ld_pw_combine forms r per element and stores the band / reduces the scores
// through the epilogue of mxa_ld_band / mxa_ld_scores itself (ld_window_store).  The band runs in groups of tile rows so that the scratch stays bounded.
// num, dx, dy are formed in fp64 from the int32 counts: every product and difference is an integer below 4 indiv^2 < 2^53 (guarded by the caller), i.e. exact
// whether or not the compiler contracts them; dx dy, the square root and the quotient are rounded once each.  The expression is symmetric in (i, j) bit for bit.
constexpr int kPwPairs = 6;
// the operand planes (A side from the I rows, B side from the J rows) of the six products, in slot order: N, Sxy, Sx, Sy, A_i.M_j, M_i.A_j
__host__ __device__ constexpr int pw_plane_a(int k) { return k == 0 ? 1 : k == 1 ? 0 : k == 2 ? 0 : k == 3 ? 1 : k == 4 ? 2 : 1; }
__host__ __device__ constexpr int pw_plane_b(int k) { return k == 0 ? 1 : k == 1 ? 0 : k == 2 ? 1 : k == 3 ? 0 : k == 4 ? 1 : 2; }

__device__ __forceinline__ double pw_r(double N, double Sxy, double Sx, double Sy, double Ax, double Ay) {
  const double Sxx = Sx + 2.0 * Ax, Syy = Sy + 2.0 * Ay;
  const double num = N * Sxy - Sx * Sy, dx = N * Sxx - Sx * Sx, dy = N * Syy - Sy * Sy;   // exact integers
  return __ddiv_rn(num, __dsqrt_rn(__dmul_rn(dx, dy)));                                    // dx dy = 0 (no shared individuals, or a SNP constant on them): 0 / 0 = NaN
}
// !SCORES: the stored entry r (ld_window_store squares it for kind 1); SCORES: the score term t(r) with the pair's own N, every operation rounded on its own.
// (ld_apply_term forms the same term under a pragma instead of these intrinsics: deliberately two, see there.)
template <bool SCORES>
__device__ __forceinline__ double pw_value(double r, double N, bool adjust) {
  if constexpr (!SCORES) return r;
  const double r2 = __dmul_rn(r, r);
  return adjust ? __dsub_rn(r2, __ddiv_rn(__dsub_rn(1.0, r2), __dsub_rn(N, 2.0))) : r2;
}

// The providers: r of one element (gi, gj) from the counts of its sub-block as ld_load_counts delivers them (cnt[slot][register]), bit for bit what the rows
// entries store at kind 0 -- and what the element's route knows besides: kSlots products per window tile, whether r is the pairwise-complete one, and then
// the pair's own N.  Plain: the LD map of xprod_store_window's fin on the one product.  Counts: pw_r of the six counts.  Sums (no missing code in the whole
// matrix): slot 0 holds Sxy only; M is all ones, so N = indiv and the other four are the per-SNP sums sz = sum z, sa = sum a (k_pw_rowsums) -- the same
// integers as the six counts, hence the same bits.
struct LdPairsPlain {
  static constexpr int kSlots = 1;
  static constexpr bool kPairwise = false;
  const double *__restrict__ u, *__restrict__ w;
  double a;
  __device__ __forceinline__ double r(const int (&cnt)[kSlots][16], int reg, long gi, long gj) const {
    return ld_scale_map(ld_center_map((double)cnt[0][reg], u[gj], u[gi], a), w[gj], w[gi]);
  }
};
struct LdPairsCounts {
  static constexpr int kSlots = kPwPairs;
  static constexpr bool kPairwise = true;
  __device__ __forceinline__ double r(const int (&cnt)[kSlots][16], int reg, long, long) const {
    return pw_r((double)cnt[0][reg], (double)cnt[1][reg], (double)cnt[2][reg], (double)cnt[3][reg], (double)cnt[4][reg], (double)cnt[5][reg]);
  }
  __device__ __forceinline__ double N(const int (&cnt)[kSlots][16], int reg) const { return (double)cnt[0][reg]; }
};
struct LdPairsSums {
  static constexpr int kSlots = 1;
  static constexpr bool kPairwise = true;
  const int *__restrict__ sz, *__restrict__ sa;
  double indiv;
  __device__ __forceinline__ double r(const int (&cnt)[kSlots][16], int reg, long gi, long gj) const {
    return pw_r(indiv, (double)cnt[0][reg], (double)sz[gi], (double)sz[gj], (double)sa[gi], (double)sa[gj]);
  }
  __device__ __forceinline__ double N(const int (&)[kSlots][16], int) const { return indiv; }
};

// One workgroup per band tile, the lane <-> element map of the crossproduct epilogue (xacc_row).  Prov: LdPairsCounts (the six counts of the tile's slots
// t.w .. t.w + 5) or LdPairsSums.  Win: the window object, by value (LdFixedWindow: the band or its scores; LdVarWindow: ragged rows or their scores).
template <bool SCORES, typename Prov, typename Win>
__global__ void __launch_bounds__(256) k_ld_pw_combine(const int *__restrict__ scratch, const int4 *__restrict__ btiles, long n, double *__restrict__ out, long ld, Prov prov,
                                                       Win win, int flag) {
  __shared__ __attribute__((aligned(16))) char smem[kXScratchBytes + (SCORES ? 2 * 4 * 2 * 4 * 32 * 8 : 0)];
  const int4 t = btiles[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wi = wave >> 1, wj = wave & 1;
  const long i0 = (long)t.x * kXT, j0 = (long)t.y * kXT;
  const int col = lane & 31, hh = lane >> 5;
  const bool adjust = flag != 0;
  int cnt[Prov::kSlots][16];                                 // the counts of the current sub-block, in accumulator register order
  long gi_base = 0, gj = 0;
  auto prep = [&](int a, int b) {
    gi_base = i0 + wi * 128 + a * 32; gj = j0 + wj * 128 + b * 32 + col;
    ld_load_counts(scratch, t.w, a, b, cnt);
  };
  auto val = [&](int, int, int r) -> double { return pw_value<SCORES>(prov.r(cnt, r, gi_base + xacc_row(r, 4 * hh), gj), prov.N(cnt, r), adjust); };
  ld_window_store<SCORES>(win, prep, val, [](double v, long, long) { return v; }, !SCORES && flag != 0, smem, wave, lane, wi, wj, i0, j0, n, out, ld);
}

// per SNP row: sz = sum z (plane Z), sa = sum a (plane A) of the stacked operand, for the missing-free path.  Grid (row tiles, K chunks), thread = row of the tile
// reading its 32-byte piece of every slab of the chunk (as k_x_rowstats); int32 atomics across the chunks (integer addition: order-independent).
__global__ void __launch_bounds__(256) k_pw_rowsums(const uint8_t *__restrict__ X, long nslabs, long slabs_per_chunk, long nb, int *__restrict__ sz, int *__restrict__ sa) {
  const long rt = blockIdx.x;
  const long s0 = (long)blockIdx.y * slabs_per_chunk, s1 = min(nslabs, s0 + slabs_per_chunk);
  int z = 0, a = 0;
  for (long sl = s0; sl < s1; sl++) {
    const uint4 *pz = reinterpret_cast<const uint4 *>(X + ((size_t)rt * nslabs + (size_t)sl) * kTileBytes + (size_t)threadIdx.x * kSlabBytes);
    const uint4 *pa = reinterpret_cast<const uint4 *>(X + ((size_t)(2 * nb + rt) * nslabs + (size_t)sl) * kTileBytes + (size_t)threadIdx.x * kSlabBytes);
    const uint4 z0 = pz[0], z1 = pz[1], a0 = pa[0], a1 = pa[1];
    const uint32_t wz[8] = {z0.x, z0.y, z0.z, z0.w, z1.x, z1.y, z1.z, z1.w}, wa[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
    for (int d = 0; d < 8; d++) {
      z += __popc(wz[d] & 0x55555555u) + 2 * __popc(wz[d] & 0xAAAAAAAAu);
      a += __popc(wa[d]);
    }
  }
  const long r = rt * kTileRows + threadIdx.x;
  if (z) atomicAdd(sz + r, z);
  if (a) atomicAdd(sa + r, a);
}

// The plan of one group of window tile rows [i_lo, i_hi): per window tile (i, j <= jmax[i]) one entry of `band` (i, j, 1, first slot) and `pairs` entries of `prod`
// over the stacked operand (plane_a nb + i, plane_b nb + j, 1, slot); slots are numbered from 0 within the group.  (miraculix_amd.crossproduct.ld_pairwise_tiles restates it.)
static void pairwise_group_tiles(int nb, const std::vector<int> &jmax, int i_lo, int i_hi, int pairs, std::vector<int4> &prod, std::vector<int4> &band) {
  int slot = 0;
  for (int i = i_lo; i < i_hi; i++)
    for (int j = i; j <= jmax[(size_t)i]; j++) {
      band.push_back(make_int4(i, j, 1, slot));
      // pairs == 1: the (Z, Z) product alone
      for (int k = 0; k < pairs; k++) prod.push_back(pairs == 1 ? make_int4(i, j, 1, slot) : make_int4(pw_plane_a(k) * nb + i, pw_plane_b(k) * nb + j, 1, slot + k));
      slot += pairs;
    }
}

// The groups of a window whose tile products go through the count scratch (the pairwise-complete entries: pairs = 6 or 1; the CSR entries of the plain route:
// pairs = 1): consecutive tile rows whose `pairs` slots of 256 KiB per window tile stay under `cap` bytes.  Fixed window: equally many rows each, sized by
// the longest tile row; general window (tile rows of different lengths): as many rows as keep the group's own tiles under the cap.  One tile row at least
// either way; the results do not depend on the groups.  Group q: tile rows [row0[q], row0[q + 1]), products prod[q], window tiles band[band_first[q] ..).
namespace {
constexpr size_t kPwSlotBytes = kPwSlotInts * sizeof(int);
static size_t ld_scratch_cap() {   // MXA_LD_PAIRWISE_SCRATCH_MB, read per call
  const char *e_cap = getenv("MXA_LD_PAIRWISE_SCRATCH_MB");
  return (size_t)(e_cap && atol(e_cap) > 0 ? atol(e_cap) : 2048L) << 20;
}
struct LdGroups {
  std::vector<int> row0;
  int n = 0;
  std::vector<std::vector<int4>> prod;
  std::vector<int4> band;
  std::vector<size_t> band_first;
  size_t tiles_max = 0;
  // tile_extra: bytes a window tile holds next to its count slots under the same cap (the partials of the apply entries)
  void plan(const LdWindow &c, size_t cap, int pairs, size_t tile_extra) {
    row0.assign(1, 0);
    const XGeom &g = c.g;
    const size_t tile_bytes = (size_t)pairs * kPwSlotBytes + tile_extra;
    if (!c.general()) {
      const int rows_per_group = (int)std::max<size_t>(1, std::min<size_t>((size_t)g.nb, cap / (c.row_tiles_max * tile_bytes)));
      for (int i = rows_per_group; i < g.nb; i += rows_per_group) row0.push_back(i);
    } else {
      const size_t cap_tiles = cap / tile_bytes;
      size_t held = 0;
      for (int i = 0; i < g.nb; i++) {
        const size_t t = (size_t)(c.jmax[(size_t)i] - i + 1);
        if (held && held + t > cap_tiles) { row0.push_back(i); held = 0; }
        held += t;
      }
    }
    n = (int)row0.size();
    row0.push_back(g.nb);
    prod.resize((size_t)n);
    band_first.assign((size_t)n + 1, 0);
    for (int q = 0; q < n; q++) {
      band_first[(size_t)q] = band.size();
      pairwise_group_tiles(g.nb, c.jmax, row0[(size_t)q], row0[(size_t)q + 1], pairs, prod[(size_t)q], band);
      tiles_max = std::max(tiles_max, band.size() - band_first[(size_t)q]);
    }
    band_first.back() = band.size();
  }
};
// the operand of the pairwise route: the three planes staged, the engine, and -- no missing code anywhere -- the per-SNP sums that replace five products
struct LdPairwiseOperand {
  bool f4 = false, dense = true;
  int pairs = kPwPairs;
  XBuf d_sums;
  int *d_sz = nullptr, *d_sa = nullptr;
  int stage(LdWindow &c, const unsigned char *plink) {
    const XGeom &g = c.g;
    hipStream_t s = c.s;
    const char *e_dense = getenv("MXA_LD_PAIRWISE_DENSE");
    if (stage_operand(plink, c.in_dev, c.row_bytes, true, g, (uint8_t *)c.d_X.p, (int *)c.d_flag.p, c.bounce, s, c.indiv)) return 1;
    int has_missing = 1;
    MXA_HIP(hipMemcpyAsync(&has_missing, c.d_flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
    MXA_HIP(hipStreamSynchronize(s));
    // no plane holds a 3: the FP4 engine is exact while 4 indiv < 2^24 (pick_engine's rule); MXA_XPROD_ENGINE=i8 forces int8
    f4 = 4 * c.indiv < (1L << 24);
    if (const char *e = getenv("MXA_XPROD_ENGINE")) { if (!strcmp(e, "i8")) f4 = false; }
    // no missing code anywhere: the (Z, Z) product alone, the rest from per-SNP sums (MXA_LD_PAIRWISE_DENSE=1 keeps the six products; bit-identical)
    dense = has_missing || (e_dense && atoi(e_dense) != 0);
    pairs = dense ? kPwPairs : 1;
    if (!dense) {
      if (d_sums.alloc(sizeof(int) * 2 * (size_t)g.rows_pad())) return 1;
      d_sz = (int *)d_sums.p; d_sa = d_sz + g.rows_pad();
      MXA_HIP(hipMemsetAsync(d_sums.p, 0, sizeof(int) * 2 * (size_t)g.rows_pad(), s));
      long spc = 0;
      const dim3 g_rows = rowstats_grid(g, &spc);
      hipLaunchKernelGGL(k_pw_rowsums, g_rows, dim3(256), 0, s, c.X(), g.nslabs, spc, (long)g.nb, d_sz, d_sa);
      MXA_HIP(hipGetLastError());
    }
    return 0;
  }
};
// One run of a window's tiles through the count scratch, for an LdWindow that has passed begin(): the pairwise-complete rows / scores and both routes of
// the pairs and apply entries.  stage() readies everything the groups need -- the operand of the route with its engine and statistics, the groups, their
// product lists and window tiles on the device, the scratch, and tfirst[I] = the window tiles in front of tile row I --, for_each_group() runs a group's
// products into the scratch and hands the group to the caller's kernels, with_provider() names the value of an element.
struct LdCountRun {
  LdWindow &c;
  const size_t cap;                          // of a group's scratch (ld_scratch_cap(), read once per call)
  bool pairwise = false, f4 = false;
  int pairs = 1;                             // products per window tile
  LdPlainOperand plain;
  LdPairwiseOperand pw;
  LdCountRun(LdWindow &c_, size_t cap_) : c(c_), cap(cap_) {}
  // The scratch term of the pre-flight: the slots of a group (and tile_extra bytes beside each tile's) are counted at the cap -- or at the one tile row it
  // cannot go below -- unless the whole window needs less.  pairs_max: before staging it is not known whether one product per tile will do.
  static size_t scratch_need(const LdWindow &c, size_t cap, int pairs_max, size_t tile_extra = 0) {
    const size_t tile_bytes = (size_t)pairs_max * kPwSlotBytes + tile_extra;
    return std::min(std::max(cap, c.row_tiles_max * tile_bytes), c.ntiles * tile_bytes);
  }
  // tile_extra: bytes a window tile holds next to its count slots under the same cap
  int stage(const unsigned char *plink, bool pairwise_, bool is_plink, const double *freq, size_t tile_extra = 0) {
    pairwise = pairwise_;
    if (pairwise ? pw.stage(c, plink) : plain.stage(c, plink, is_plink, freq)) return 1;
    f4 = pairwise ? pw.f4 : plain.f4;
    pairs = pairwise ? pw.pairs : 1;
    gr.plan(c, cap, pairs, tile_extra);
    const int nb = c.g.nb;
    tfirst.assign((size_t)nb + 1, 0);
    for (int I = 0; I < nb; I++) tfirst[(size_t)I + 1] = tfirst[(size_t)I] + (c.jmax[(size_t)I] - I + 1);
    if (upload_tiles(std::move(gr.prod), c.s, t)) return 1;
    if (d_bt.alloc(gr.band.size() * sizeof(int4)) || d_scr.alloc(gr.tiles_max * (size_t)pairs * kPwSlotBytes) || d_tf.alloc(sizeof(long) * tfirst.size())) return 1;
    MXA_HIP(hipMemcpyAsync(d_bt.p, gr.band.data(), gr.band.size() * sizeof(int4), hipMemcpyHostToDevice, c.s));
    MXA_HIP(hipMemcpyAsync(d_tf.p, tfirst.data(), sizeof(long) * tfirst.size(), hipMemcpyHostToDevice, c.s));
    return 0;
  }
  int ngroups() const { return gr.n; }
  int first_group_rows() const { return gr.row0[1]; }
  size_t tiles_max() const { return gr.tiles_max; }                // window tiles of the largest group
  const int *counts() const { return (const int *)d_scr.p; }       // the scratch: `pairs` slots per window tile of the current group
  const long *d_tfirst() const { return (const long *)d_tf.p; }
  // body(q, tiles, bt, i_lo, i_hi) for every group q, behind the group's products on the call's stream (the next group reuses the scratch): its `tiles`
  // window tiles bt[] = (i, j, 1, first slot) of the tile rows [i_lo, i_hi).  body returns non-zero to give up.
  template <typename Body>
  int for_each_group(Body body) {
    const XPost none{};
    for (int q = 0; q < gr.n; q++) {
      if (t.launch(q, c.g, f4, c.s, c.X(), (double *)d_scr.p, 0, 0, nullptr, kPostCounts, none)) return 1;
      if (body(q, (unsigned)(gr.band_first[(size_t)q + 1] - gr.band_first[(size_t)q]), (const int4 *)d_bt.p + gr.band_first[(size_t)q], gr.row0[(size_t)q], gr.row0[(size_t)q + 1]))
        return 1;
      MXA_HIP(hipGetLastError());
    }
    return 0;
  }
  // f(the provider of the staged route)
  template <typename F>
  auto with_provider(F f) const {
    if (!pairwise) return f(LdPairsPlain{plain.xp.u, plain.xp.w, plain.xp.a});
    if (pw.dense) return f(LdPairsCounts{});
    return f(LdPairsSums{pw.d_sz, pw.d_sa, (double)c.indiv});
  }

 private:
  LdGroups gr;
  std::vector<long> tfirst;
  XTiles t;
  XBuf d_bt, d_scr, d_tf;
};
}  // namespace

// the pairwise route: the three planes staged, per group of tile rows the count products and their combine
int ld_pairwise_any(const char *who, const unsigned char *plink, long snps, long indiv, long window, const int *last, double *out, long ldb, bool scores, int flag) {
  const size_t cap = ld_scratch_cap();
  LdWindow c(who, plink, snps, indiv, window, last, out, ldb, scores, flag);
  if (c.begin(3, [&] { return LdCountRun::scratch_need(c, cap, kPwPairs); }, nullptr, kPwMaxIndiv, "%s: the adjusted estimator r^2 - (1 - r^2) / (N - 2) needs indiv >= 3",
              "%s: at most %ld SNPs per call")) return 1;
  LdCountRun run(c, cap);
  if (run.stage(plink, true, true, nullptr) || c.start()) return 1;
  // the instantiation for (scores, provider, window object)
  auto combine = [&](unsigned tiles, const int4 *bt, auto win) {
    run.with_provider([&](auto prov) {
      using Prov = decltype(prov);
      using Win = decltype(win);
      if constexpr (Prov::kPairwise) {
        auto go = [&](auto k) { hipLaunchKernelGGL(k, dim3(tiles), dim3(256), 0, c.s, run.counts(), bt, snps, c.d_dst, c.ld_dst, prov, win, flag); };
        if (scores) go(k_ld_pw_combine<true, Prov, Win>); else go(k_ld_pw_combine<false, Prov, Win>);
      }
    });
  };
  if (run.for_each_group([&](int, unsigned tiles, const int4 *bt, int, int) {
        if (c.general()) combine(tiles, bt, LdVarWindow{(const int *)c.d_last.p, (const long *)c.d_rowptr.p, c.ndiag});
        else combine(tiles, bt, LdFixedWindow{window});
        return 0;
      })) return 1;
  if (c.finish()) return 1;
  debug_info("%s: %d group(s) of up to %d tile rows, %d product(s) per band tile (%s), %s engine", who, run.ngroups(), run.first_group_rows(), run.pairs,
             run.pw.dense ? "six counts" : "no missing code: per-SNP sums", run.f4 ? "FP4" : "int8");
  return 0;
}

// ---- pairs above a cutoff as CSR (mxa_ld_window_pairs, mxa_ld_window_pairs_pairwise): the candidates i < j <= last[i] whose q = fl(r r) >= min_r2, compacted
// on the device.  Both routes run the window's tile products once into the count scratch (kPostCounts; the plain route one slot per window tile), in the
// groups of LdGroups; per group k_ld_select counts (WRITE = false), the scan kernels turn the counts into positions, and k_ld_select runs again and writes
// (WRITE = true), recomputing its masks from the scratch, which is still in place.  Every position is a sum of counts in a fixed order: no atomics.
// The one decision of both passes: q = fl(r r), kept iff q >= min_r2 (a NaN r: the comparison is false).  Nothing here can be contracted.
__device__ __forceinline__ bool ld_pair_keep(double r, double min_r2, double &q) {
  q = __dmul_rn(r, r);
  return q >= min_r2;
}

// One workgroup per window tile.  Element (gi, gj) of the tile is held by the lane the crossproduct epilogue gives it: lane & 31 runs along gj, the two 32-lane
// halves of a wave hold rows 4 apart, so a ballot is two 32-bit words of the table mask[row][word], word = the row's 32-column sub-block, ascending in gj.
// Count pass: cnt[tile][row] = the row's popcount.  Write pass: cnt holds rel[tile][row], the row's kept pairs in the tiles to the left (k_ld_pairs_rowscan);
// position = rowptr[gi] + rel + popcounts of the row's lower words + of its own word below the lane; a position >= capacity is dropped.
// val == nullptr (the selection entries, which need the graph alone): the write pass still rebuilds its masks from the counts in the first loop; its
// second loop stores col only and skips the reload of the counts and the second evaluation of r.
template <bool WRITE, typename Prov, typename Win>
__global__ void __launch_bounds__(256) k_ld_select(const int *__restrict__ scratch, const int4 *__restrict__ btiles, long n, Prov prov, Win win, double min_r2, int kind,
                                                   int *__restrict__ cnt, const long *__restrict__ rowptr, int *__restrict__ col, double *__restrict__ val, long capacity) {
  __shared__ unsigned mask[kXT][8];
  __shared__ int below[WRITE ? kXT : 1][8];                  // kept pairs of the row in its lower words
  __shared__ long base[WRITE ? kXT : 1];                     // rowptr[gi] + rel
  const int4 t = btiles[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wi = wave >> 1, wj = wave & 1;
  const long i0 = (long)t.x * kXT, j0 = (long)t.y * kXT;
  const int c = lane & 31, hh = lane >> 5;
  int counts[Prov::kSlots][16];                              // the counts of the current sub-block, in accumulator register order
#pragma unroll
  for (int k = 0; k < 8; k++) mask[tid][k] = 0u;             // sub-blocks skipped below keep no pair
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const long gi_base = i0 + wi * 128 + a * 32, gj_base = j0 + wj * 128 + b * 32;
      if (gj_base + 31 <= gi_base || win.beyond(gi_base, gj_base, n)) continue;   // wave-uniform: no element above the diagonal, or none within the window
      ld_load_counts(scratch, t.w, a, b, counts);
      const long gj = gj_base + c;
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const int row = xacc_row(reg, 4 * hh);
        const long gi = gi_base + row;
        bool keep = false;
        if (gi < gj && gj < n && win.in(gi, gj)) {
          double q;
          keep = ld_pair_keep(prov.r(counts, reg, gi, gj), min_r2, q);
        }
        const unsigned long long bal = __ballot(keep);
        if (c == 0) mask[wi * 128 + a * 32 + row][wj * 4 + b] = (unsigned)(bal >> (32 * hh));
      }
    }
  __syncthreads();
  int *mine = cnt + (size_t)blockIdx.x * kXT + tid;
  if constexpr (!WRITE) {
    int total = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) total += __popc(mask[tid][k]);
    *mine = total;
  } else {
    int run = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) { below[tid][k] = run; run += __popc(mask[tid][k]); }
    base[tid] = i0 + tid < n ? rowptr[i0 + tid] + (long)*mine : 0L;
    const bool want_val = val != nullptr;
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const long gi_base = i0 + wi * 128 + a * 32, gj_base = j0 + wj * 128 + b * 32;
        if (gj_base + 31 <= gi_base || win.beyond(gi_base, gj_base, n)) continue;
        if (want_val) ld_load_counts(scratch, t.w, a, b, counts);
        const long gj = gj_base + c;
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
          const int row = wi * 128 + a * 32 + xacc_row(reg, 4 * hh), word = wj * 4 + b;
          const unsigned m = mask[row][word];
          if ((m >> c) & 1u) {                               // kept by the decision above: gi < gj < n
            const long pos = base[row] + (long)(below[row][word] + __popc(m & ((1u << c) - 1u)));
            if (pos < capacity) {
              col[pos] = (int)gj;
              if (want_val) {
                double q;
                const double r = prov.r(counts, reg, i0 + row, gj);
                ld_pair_keep(r, min_r2, q);
                val[pos] = kind ? q : r;
              }
            }
          }
        }
      }
  }
}

// Between the two passes of a group: one workgroup per tile row I = i_lo + blockIdx.x of the group, thread = row.  cnt over the row's tiles (J ascending,
// tfirst[I] = the window tiles in front of tile row I) becomes the exclusive offsets rel; the row totals are scanned within the tile row (rowptr[gi] = the
// offset inside the tile row for now) and the tile row's total goes to rowsum[blockIdx.x].
__global__ void __launch_bounds__(256) k_ld_pairs_rowscan(int *__restrict__ cnt, const long *__restrict__ tfirst, int i_lo, long n, long *__restrict__ rowptr,
                                                          long *__restrict__ rowsum) {
  __shared__ long sc[kXT];
  const int tid = threadIdx.x, I = i_lo + (int)blockIdx.x;
  const long t0 = tfirst[I] - tfirst[i_lo], t1 = tfirst[I + 1] - tfirst[i_lo];
  int run = 0;                                               // < n: fits an int
  for (long t = t0; t < t1; t++) {
    int *p = cnt + (size_t)t * kXT + tid;
    const int v = *p;
    *p = run;
    run += v;
  }
  sc[tid] = run;
  __syncthreads();
  for (int off = 1; off < kXT; off <<= 1) {
    const long v = tid >= off ? sc[tid - off] : 0L;
    __syncthreads();
    sc[tid] += v;
    __syncthreads();
  }
  const long gi = (long)I * kXT + tid;
  if (gi < n) rowptr[gi] = sc[tid] - run;
  if (tid == kXT - 1) rowsum[blockIdx.x] = sc[tid];
}
// One workgroup: rowsum[0 .. nrows) of the group's tile rows -> their exclusive prefix sums from the running base *base (the pairs of all earlier groups), and
// *base moves on by the group's total.  Thread t sums a run of consecutive tile rows, the runs are scanned through the LDS.
__global__ void __launch_bounds__(1024) k_ld_pairs_groupscan(long *__restrict__ rowsum, int nrows, long *__restrict__ base) {
  __shared__ long sc[1024];
  const int tid = threadIdx.x, per = (nrows + 1023) / 1024, r0 = min(nrows, tid * per), r1 = min(nrows, r0 + per);
  const long start = *base;
  long run = 0;
  for (int r = r0; r < r1; r++) run += rowsum[r];
  sc[tid] = run;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const long v = tid >= off ? sc[tid - off] : 0L;
    __syncthreads();
    sc[tid] += v;
    __syncthreads();
  }
  long at = start + sc[tid] - run;
  for (int r = r0; r < r1; r++) { const long v = rowsum[r]; rowsum[r] = at; at += v; }
  if (tid == 1023) *base = start + sc[tid];
}
// rowptr[gi] of the group's rows: the offset inside the tile row plus the tile row's start; behind the last group rowptr[n] = the total
__global__ void __launch_bounds__(256) k_ld_pairs_rowptr(long *__restrict__ rowptr, const long *__restrict__ rowstart, int i_lo, long n, const long *__restrict__ base, int is_last) {
  const long gi = ((long)i_lo + blockIdx.x) * kXT + threadIdx.x;
  if (gi < n) rowptr[gi] += rowstart[blockIdx.x];
  if (is_last && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) rowptr[n] = *base;
}

// both routes of the CSR entries (pairwise: the pairwise-complete r; else the plain route with is_plink and freq).  no_val: the library's own filling call
// with col alone (ld_prune_window); the public entries pass false and reject a lone NULL.
int ld_pairs_any(const char *who, const unsigned char *plink, long snps, long indiv, const int *last, double min_r2, int kind, long *rowptr, int *col, double *val,
                        long capacity, long *total, bool pairwise, bool is_plink, const double *freq, bool no_val) {
  if (!last || !rowptr || !total) { set_error(1, "%s: bad arguments", who); return 1; }
  if (!no_val && (col == nullptr) != (val == nullptr)) { set_error(1, "%s: col and val must both be given (the filling call) or both be NULL (the count-only call)", who); return 1; }
  if (col && capacity < 0) { set_error(1, "%s: capacity must not be negative (%ld)", who, capacity); return 1; }
  if (!(min_r2 >= 0.0) || min_r2 > DBL_MAX) { set_error(1, "%s: min_r2 must be finite and not negative", who); return 1; }
  const size_t cap = ld_scratch_cap();
  LdWindow c(who, plink, snps, indiv, 0, last, reinterpret_cast<double *>(rowptr), 0, false, kind);
  c.set_pairs(col, val, capacity, total);
  // the scratch, the per-(tile, row) counters of a group (1 KiB per window tile), and per tile row tfirst and the row sums
  auto extra = [&] {
    return LdCountRun::scratch_need(c, cap, pairwise ? kPwPairs : 1) + std::min(c.ntiles, std::max(cap / kPwSlotBytes, c.row_tiles_max)) * kXT * sizeof(int) +
           sizeof(long) * (2 * (size_t)c.g.nb + 2);
  };
  if (c.begin(pairwise ? 3 : 1, extra, pairwise || freq ? nullptr : "%s: allele frequencies are required", pairwise ? kPwMaxIndiv : 0L, "%s",
              pairwise ? "%s: at most %ld SNPs per call" : "%s: at most %ld SNPs per call (the fused statistics)")) return 1;
  hipStream_t s = c.s;
  LdCountRun run(c, cap);
  if (run.stage(plink, pairwise, is_plink, freq)) return 1;
  XBuf d_cnt, d_rows;                                        // d_rows: the groups' row sums (nb longs), the running base (1)
  if (d_cnt.alloc(run.tiles_max() * kXT * sizeof(int)) || d_rows.alloc(sizeof(long) * ((size_t)c.g.nb + 1))) return 1;
  long *d_rowsum = (long *)d_rows.p, *d_base = d_rowsum + c.g.nb;
  MXA_HIP(hipMemsetAsync(d_base, 0, sizeof(long), s));
  if (c.start()) return 1;
  const LdVarWindow win{(const int *)c.d_last.p, nullptr, c.ndiag};
  long *d_rowptr = c.d_pairs_rowptr();
  // per group: count; scan (the running base crosses the groups on the device: the host does not wait); write
  if (run.for_each_group([&](int q, unsigned tiles, const int4 *bt, int i_lo, int i_hi) {
        const int nrows = i_hi - i_lo;
        auto pass = [&](auto write) {
          run.with_provider([&](auto prov) {
            hipLaunchKernelGGL((k_ld_select<decltype(write)::value, decltype(prov), LdVarWindow>), dim3(tiles), dim3(256), 0, s, run.counts(), bt, snps, prov, win, min_r2, kind,
                               (int *)d_cnt.p, (const long *)d_rowptr, c.d_pairs_col(), c.d_pairs_val(), c.capacity);
          });
        };
        pass(std::false_type());
        hipLaunchKernelGGL(k_ld_pairs_rowscan, dim3((unsigned)nrows), dim3(256), 0, s, (int *)d_cnt.p, run.d_tfirst(), i_lo, snps, d_rowptr, d_rowsum);
        hipLaunchKernelGGL(k_ld_pairs_groupscan, dim3(1), dim3(1024), 0, s, d_rowsum, nrows, d_base);
        hipLaunchKernelGGL(k_ld_pairs_rowptr, dim3((unsigned)nrows), dim3(256), 0, s, d_rowptr, (const long *)d_rowsum, i_lo, snps, (const long *)d_base, q == run.ngroups() - 1 ? 1 : 0);
        if (c.result == LdResult::kPairsFill) pass(std::true_type());
        return 0;
      })) return 1;
  if (c.finish(d_base)) return 1;
  debug_info("%s: %d group(s), %d product(s) per window tile, %s engine, %ld pairs", who, run.ngroups(), run.pairs, run.f4 ? "FP4" : "int8", *total);
  return 0;
}

// ---- the window applied to a matrix (mxa_ld_window_apply, mxa_ld_window_apply_pairwise): Y = T_w(R) X, Y[i, c] = sum over first[i] <= j <= last[i] of
// t(r_ij) X[j, c], X and Y snps x n column-major.  Neither the rows nor the band are written: both routes run the window's tile products once into the count
// scratch (kPostCounts, the groups of LdGroups, as the CSR entries do), k_ld_apply_tile turns every window tile into two partials per chunk of kLdApplyNC
// columns -- the I side P_I[i][c] = sum_j t_ij X[j, c] over the tile's elements i <= j, the J side P_J[j][c] = sum_i t_ij X[i, c] over its elements i < j --
// and k_ld_apply_finish adds the partials of a group to Y in the canonical order of a row block B: the J sides of the tiles (I, B), I ascending, then the I
// sides of the tiles (B, J), J ascending.  Groups are consecutive tile rows and the running sum passes through Y between them, so the association of every
// sum is the same for every group partition; inside a tile the order is fixed by the lane <-> element map alone and every column runs the same
// instructions, so it does not depend on the engine, on where the pointers live, on the scratch size or on n.  No floating-point atomics.
// t: term 0 = r, the providers' value (bit for bit what the rows entries store at kind 0); 1 = fl(r r); 2 = the adjusted term of the scores entries -- the
// plain route r2 - (1 - r2) (1 / (indiv - 2)) as xprod_store_window forms it, the pairwise route with the pair's own N as pw_value<true> does.
constexpr int kLdApplyNC = 16;                                          // columns of X per workgroup
constexpr int kLdApplyXBytes = 2 * kXT * kLdApplyNC * 8;                // xs[side][row][NC]: the X rows of tile rows I and J; afterwards the two halves of a side's partial
constexpr int kLdApplyLds = kLdApplyXBytes + kXScratchBytes + 4 * 32 * 4;   // + the four waves' 32 x 33 sub-block of t and their 32 row masks: 99 840 bytes
constexpr long kLdApplyMaxCols = 65535L * kLdApplyNC;                   // grid.y

template <typename Prov>
__device__ __forceinline__ double ld_apply_term(const Prov &prov, const int (&cnt)[Prov::kSlots][16], int reg, long gi, long gj, int term, double inv_adj) {
  // Every operation below is rounded on its own.  They are written as operators under this pragma and not as __dmul_rn / __dsub_rn: those are plain operators
  // inside the toolchain's header, compiled there with contraction allowed, and once inlined the compiler fuses r r - p or r2 - q g into an fma all the same.
#pragma clang fp contract(off)
  const double r = prov.r(cnt, reg, gi, gj);
  if (term == 0) return r;
  const double r2 = r * r;
  if (term == 1) return r2;
  const double q = 1.0 - r2;
  if constexpr (!Prov::kPairwise) {
    const double p = q * inv_adj;
    return r2 - p;
  } else {
    const double p = q / (prov.N(cnt, reg) - 2.0);
    return r2 - p;
  }
}

// Grid (window tiles of the group, column chunks).  The counts are read with the lane <-> element map of k_ld_select; a wave takes its 128 x 128 quadrant
// sub-block by sub-block: t of the 32 x 32 sub-block goes to the wave's padded LDS scratch (0 outside the window) and the row masks of the ballot say which
// elements count -- an element outside the window is skipped, not multiplied.  Then lane (c = lane & 31, hh = lane >> 5) owns the 8 columns 8 hh .. 8 hh + 7
// of the chunk: for the J side it is column gj_base + c and walks the 32 rows of the sub-block (X[gi, .] an LDS broadcast), for the I side it is row
// gi_base + c and walks the 32 columns (t read transposed, stride 33).  A lane's sum runs over rows / columns ascending within a sub-block and over the
// sub-blocks a (b) ascending; the two waves that share rows (columns) are added as wj = 0 + wj = 1 (wi = 0 + wi = 1) through the LDS.
template <typename Prov, typename Win>
__global__ void __launch_bounds__(256) k_ld_apply_tile(const int *__restrict__ scratch, const int4 *__restrict__ btiles, long n, Prov prov, Win win, int term,
                                                       const double *__restrict__ X, long ldx, int ncols, double *__restrict__ P) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NC = kLdApplyNC;
  const int4 t = btiles[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wi = wave >> 1, wj = wave & 1;
  const int c = lane & 31, hh = lane >> 5, kh = 8 * hh;
  const long i0 = (long)t.x * kXT, j0 = (long)t.y * kXT;
  const int c0 = (int)blockIdx.y * NC;
  double *xs = reinterpret_cast<double *>(smem);
  double *tsc = reinterpret_cast<double *>(smem + kLdApplyXBytes) + wave * (32 * 33);
  unsigned *rmask = reinterpret_cast<unsigned *>(smem + kLdApplyXBytes + kXScratchBytes) + wave * 32;
  double inv_adj = 0.0;
  if constexpr (!Prov::kPairwise) inv_adj = term == 2 ? 1.0 / (prov.a * 0.25 - 2.0) : 0.0;   // prov.a = 4 indiv
  for (int e = tid; e < 2 * kXT * NC; e += 256) {           // e = (side NC + k) 256 + row: the threads run along the rows of a column of X
    const int row = e & (kXT - 1), k = (e >> 8) % NC, side = e / (kXT * NC);
    const long g = (side ? j0 : i0) + row;
    xs[(side * kXT + row) * NC + k] = g < n && c0 + k < ncols ? X[(size_t)g + (size_t)(c0 + k) * (size_t)ldx] : 0.0;
  }
  __syncthreads();
  int counts[Prov::kSlots][16];                              // the counts of the current sub-block, in accumulator register order
  double rowacc[4][8], colacc[4][8];
#pragma unroll
  for (int q = 0; q < 4; q++)
#pragma unroll
    for (int k = 0; k < 8; k++) rowacc[q][k] = colacc[q][k] = 0.0;
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const long gi_base = i0 + wi * 128 + a * 32, gj_base = j0 + wj * 128 + b * 32;
      if (gj_base + 31 < gi_base || win.beyond(gi_base, gj_base, n)) continue;   // wave-uniform: wholly below the diagonal, or no element within the window
      ld_load_counts(scratch, t.w, a, b, counts);
      const long gj = gj_base + c;
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const int row = xacc_row(reg, 4 * hh);
        const long gi = gi_base + row;
        const bool ok = gi <= gj && gj < n && win.in(gi, gj);
        double tv = 0.0;
        if (ok) tv = ld_apply_term(prov, counts, reg, gi, gj, term, inv_adj);
        tsc[row * 33 + c] = tv;
        const unsigned long long bal = __ballot(ok);
        if (c == 0) rmask[row] = (unsigned)(bal >> (32 * hh));
      }
      __builtin_amdgcn_wave_barrier();                       // the wave reads what it wrote: LDS operations of one wave complete in order
      // J side: column gj, the rows gi < gj of the sub-block
      const double *xi = xs + ((wi * 128 + a * 32) * NC + kh);
#pragma unroll 2
      for (int row = 0; row < 32; row++) {
        if (((rmask[row] >> c) & 1u) && gi_base + row != gj) {
          const double tv = tsc[row * 33 + c];
#pragma unroll
          for (int k = 0; k < 8; k++) colacc[b][k] = fma(tv, xi[row * NC + k], colacc[b][k]);
        }
      }
      // I side: row gi_base + c, the columns of the sub-block
      const unsigned mine = rmask[c];
      const double *xj = xs + ((kXT + wj * 128 + b * 32) * NC + kh);
#pragma unroll 2
      for (int cc = 0; cc < 32; cc++) {
        if ((mine >> cc) & 1u) {
          const double tv = tsc[c * 33 + cc];
#pragma unroll
          for (int k = 0; k < 8; k++) rowacc[a][k] = fma(tv, xj[cc * NC + k], rowacc[a][k]);
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  // the partials of the tile: P[tile][side][row][ncols]; a side is the sum of its two halves, formed through the LDS where X was
  double *Pt = P + (size_t)blockIdx.x * 2 * kXT * (size_t)ncols;
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int k = 0; k < 8; k++) xs[(wj * kXT + wi * 128 + a * 32 + c) * NC + kh + k] = rowacc[a][k];
  __syncthreads();
  for (int e = tid; e < kXT * NC; e += 256) {
    const int row = e / NC, k = e % NC;
    if (c0 + k < ncols) Pt[(size_t)row * (size_t)ncols + (size_t)(c0 + k)] = xs[row * NC + k] + xs[(kXT + row) * NC + k];
  }
  __syncthreads();
#pragma unroll
  for (int b = 0; b < 4; b++)
#pragma unroll
    for (int k = 0; k < 8; k++) xs[(wi * kXT + wj * 128 + b * 32 + c) * NC + kh + k] = colacc[b][k];
  __syncthreads();
  for (int e = tid; e < kXT * NC; e += 256) {
    const int row = e / NC, k = e % NC;
    if (c0 + k < ncols) Pt[(size_t)(kXT + row) * (size_t)ncols + (size_t)(c0 + k)] = xs[row * NC + k] + xs[(kXT + row) * NC + k];
  }
}

// Per group of tile rows [i_lo, i_hi): one thread per (row i, column c) of the row blocks B = i_lo .. jmax[i_hi - 1] the group touches.  Y[i, c] takes, in this
// order, the J sides of the group's tiles (I, B), I ascending from max(i_lo, imin[B]) (imin[B] = the first tile row that reaches B; jmax is non-decreasing),
// and, where B is one of the group's tile rows, the I sides of its tiles (B, J), J ascending.  tfirst[I] = the window tiles in front of tile row I.
__global__ void __launch_bounds__(256) k_ld_apply_finish(const double *__restrict__ P, int ncols, const long *__restrict__ tfirst, const int *__restrict__ jmax,
                                                         const int *__restrict__ imin, int i_lo, int i_hi, long n, long nrows, double *__restrict__ Y, long ldy,
                                                         long blk0) {
  const long idx = (blk0 + blockIdx.x) * 256 + threadIdx.x;
  if (idx >= nrows * (long)ncols) return;
  const long i = (long)i_lo * kXT + idx / ncols;
  const int col = (int)(idx % ncols);
  if (i >= n) return;
  const int B = (int)(i / kXT), rr = (int)(i % kXT);
  double *y = Y + (size_t)i + (size_t)col * (size_t)ldy;
  double sum = *y;
  auto part = [&](long tile, int side) { return P[((size_t)(tile * 2 + side) * kXT + (size_t)rr) * (size_t)ncols + (size_t)col]; };
  const int i_end = min(i_hi - 1, B);
  for (int I = max(i_lo, imin[B]); I <= i_end; I++) sum += part(tfirst[I] - tfirst[i_lo] + (B - I), 1);
  if (B < i_hi) {
    const int J1 = jmax[B];
    for (int J = B; J <= J1; J++) sum += part(tfirst[B] - tfirst[i_lo] + (J - B), 0);
  }
  *y = sum;
}

// both routes of the apply entries (pairwise: the pairwise-complete r; else the plain route with is_plink and freq)
static int ld_apply_any(const char *who, const unsigned char *plink, long snps, long indiv, const int *last, int term, const double *X, long ldx, long n, double *Y,
                        long ldy, bool pairwise, bool is_plink, const double *freq) {
  if (!last || !X || !Y) { set_error(1, "%s: bad arguments", who); return 1; }
  if (n < 1 || n > kLdApplyMaxCols) { set_error(1, "%s: need 1 <= n <= %ld (n %ld)", who, kLdApplyMaxCols, n); return 1; }
  if (term < 0 || term > 2) { set_error(1, "%s: term must be 0, 1 or 2", who); return 1; }
  if (term == 2 && indiv < 3) { set_error(1, "%s: the adjusted term needs indiv >= 3", who); return 1; }
  if (snps > 0 && (ldx < snps || ldy < snps)) { set_error(1, "%s: need ldx >= snps and ldy >= snps (ldx %ld, ldy %ld, snps %ld)", who, ldx, ldy, snps); return 1; }
  const size_t cap = ld_scratch_cap();
  LdWindow c(who, plink, snps, indiv, 0, last, Y, ldy, false, 0);
  c.set_apply((int)n);
  const size_t part_bytes = sizeof(double) * 2 * kXT * (size_t)n;   // the partials of a window tile: they share the cap with its count slots
  bool x_dev = false;
  // the scratch and the partials, the device copy of a host X, the window tiles' list and the plan's arrays
  auto extra = [&] {
    x_dev = ptr_location(X, nullptr) == 1;
    return LdCountRun::scratch_need(c, cap, pairwise ? kPwPairs : 1, part_bytes) + (x_dev ? 0 : sizeof(double) * (size_t)snps * (size_t)n) + c.ntiles * sizeof(int4) +
           sizeof(long) * ((size_t)c.g.nb + 1) + 2 * sizeof(int) * (size_t)c.g.nb;
  };
  if (c.begin(pairwise ? 3 : 1, extra, pairwise || freq ? nullptr : "%s: allele frequencies are required", pairwise ? kPwMaxIndiv : 0L, "%s",
              pairwise ? "%s: at most %ld SNPs per call" : "%s: at most %ld SNPs per call (the fused statistics)")) return 1;
  const XGeom &g = c.g;
  hipStream_t s = c.s;
  LdCountRun run(c, cap);
  if (run.stage(plink, pairwise, is_plink, freq, part_bytes)) return 1;
  // the plan's arrays on the device: jmax and imin (nb ints each)
  std::vector<int> imin((size_t)g.nb, 0);
  for (int B = 0, I = 0; B < g.nb; B++) { while (c.jmax[(size_t)I] < B) I++; imin[(size_t)B] = I; }   // jmax[B] >= B ends the search
  XBuf d_part, d_plan, d_xm;
  if (d_part.alloc(run.tiles_max() * part_bytes) || d_plan.alloc(2 * sizeof(int) * (size_t)g.nb) || (!x_dev && d_xm.alloc(sizeof(double) * (size_t)snps * (size_t)n))) return 1;
  int *d_jmax = (int *)d_plan.p, *d_imin = d_jmax + g.nb;
  MXA_HIP(hipMemcpyAsync(d_jmax, c.jmax.data(), sizeof(int) * (size_t)g.nb, hipMemcpyHostToDevice, s));
  MXA_HIP(hipMemcpyAsync(d_imin, imin.data(), sizeof(int) * (size_t)g.nb, hipMemcpyHostToDevice, s));
  // X once to the device (compact), Y cleared once: its snps rows of every column, nothing else
  const double *d_x = X;
  long ld_x = ldx;
  if (!x_dev) {
    MXA_HIP(hipMemcpy2DAsync(d_xm.p, sizeof(double) * (size_t)snps, X, sizeof(double) * (size_t)ldx, sizeof(double) * (size_t)snps, (size_t)n, hipMemcpyHostToDevice, s));
    d_x = (const double *)d_xm.p;
    ld_x = snps;
  }
  double *d_y = c.d_res;
  const long ld_y = c.out_dev ? ldy : snps;
  MXA_HIP(hipMemset2DAsync(d_y, sizeof(double) * (size_t)ld_y, 0, sizeof(double) * (size_t)snps, (size_t)n, s));
  if (c.start()) return 1;
  const LdVarWindow win{(const int *)c.d_last.p, nullptr, c.ndiag};
  const unsigned chunks = (unsigned)((n + kLdApplyNC - 1) / kLdApplyNC);
  // per group: its tiles' partials, and the partials into Y (the next group reuses the scratch and the partials)
  if (run.for_each_group([&](int, unsigned tiles, const int4 *bt, int i_lo, int i_hi) {
        if (run.with_provider([&](auto prov) {
              constexpr auto K = &k_ld_apply_tile<decltype(prov), LdVarWindow>;
              static unsigned long long lds_mask = 0;        // per instantiation
              if (ensure_dyn_lds(reinterpret_cast<const void *>(K), kLdApplyLds, &lds_mask)) return 1;
              hipLaunchKernelGGL(K, dim3(tiles, chunks), dim3(256), kLdApplyLds, s, run.counts(), bt, snps, prov, win, term, d_x, ld_x, (int)n, (double *)d_part.p);
              return 0;
            })) return 1;
        const long nrows = std::min(snps, ((long)c.jmax[(size_t)i_hi - 1] + 1) * kXT) - (long)i_lo * kXT;
        // One thread per (row, column) of the group: the limit of a launch is 2^32 threads, not 2^31 workgroups, so this goes in pieces as well (every thread
        // owns its Y[i, c]: no order between the pieces).  No test reaches the second piece: under the default 2 GiB scratch cap a group holds nrows n <= 2^26,
        // and 2^32 (row, column) pairs in one group need more than 100 GB of partial sums.
        launch_in_block_chunks((nrows * n + 255) / 256, [&](unsigned nb, long blk0) {
          hipLaunchKernelGGL(k_ld_apply_finish, dim3(nb), dim3(256), 0, s, (const double *)d_part.p, (int)n, run.d_tfirst(), (const int *)d_jmax, (const int *)d_imin, i_lo, i_hi,
                             snps, nrows, d_y, ld_y, blk0);
        });
        return 0;
      })) return 1;
  if (c.finish()) return 1;
  debug_info("%s: %d group(s), %d product(s) per window tile, %s engine, %ld column(s) in %u chunk(s)", who, run.ngroups(), run.pairs, run.f4 ? "FP4" : "int8", n, chunks);
  return 0;
}

}  // namespace mxa

extern "C" int mxa_ld_band_pairwise(const unsigned char *plink, int snps, int indiv, int window, double *band, long ldb, int kind) {
  mxa::clear_error();
  return mxa::ld_pairwise_any("mxa_ld_band_pairwise", plink, snps, indiv, window, nullptr, band, ldb, false, kind);
}

extern "C" int mxa_ld_scores_pairwise(const unsigned char *plink, int snps, int indiv, int window, double *scores, int adjust) {
  mxa::clear_error();
  return mxa::ld_pairwise_any("mxa_ld_scores_pairwise", plink, snps, indiv, window, nullptr, scores, 0, true, adjust);
}

extern "C" int mxa_ld_band(const unsigned char *plink, int snps, int indiv, int window, double *band, long ldb, int kind, int is_plink_format,
                           const double *allele_freq) {
  mxa::clear_error();
  return mxa::ld_window_any("mxa_ld_band", plink, snps, indiv, window, nullptr, band, ldb, false, kind, is_plink_format != 0, allele_freq);
}

extern "C" int mxa_ld_scores(const unsigned char *plink, int snps, int indiv, int window, double *scores, int adjust, int is_plink_format,
                             const double *allele_freq) {
  mxa::clear_error();
  return mxa::ld_window_any("mxa_ld_scores", plink, snps, indiv, window, nullptr, scores, 0, true, adjust, is_plink_format != 0, allele_freq);
}

// ---- windowed LD by distance: the window of SNP i ends at last[i] (mxa_ld_window_bounds makes it from base pairs / centimorgans / SNP counts and chromosomes)
extern "C" int mxa_ld_window_rows(const unsigned char *plink, int snps, int indiv, const int *last, double *rows, int kind, int is_plink_format, const double *allele_freq) {
  mxa::clear_error();
  if (!last) { mxa::set_error(1, "mxa_ld_window_rows: bad arguments"); return 1; }
  return mxa::ld_window_any("mxa_ld_window_rows", plink, snps, indiv, 0, last, rows, 0, false, kind, is_plink_format != 0, allele_freq);
}

extern "C" int mxa_ld_window_scores(const unsigned char *plink, int snps, int indiv, const int *last, double *scores, int adjust, int is_plink_format,
                                    const double *allele_freq) {
  mxa::clear_error();
  if (!last) { mxa::set_error(1, "mxa_ld_window_scores: bad arguments"); return 1; }
  return mxa::ld_window_any("mxa_ld_window_scores", plink, snps, indiv, 0, last, scores, 0, true, adjust, is_plink_format != 0, allele_freq);
}

extern "C" int mxa_ld_window_rows_pairwise(const unsigned char *plink, int snps, int indiv, const int *last, double *rows, int kind) {
  mxa::clear_error();
  if (!last) { mxa::set_error(1, "mxa_ld_window_rows_pairwise: bad arguments"); return 1; }
  return mxa::ld_pairwise_any("mxa_ld_window_rows_pairwise", plink, snps, indiv, 0, last, rows, 0, false, kind);
}

extern "C" int mxa_ld_window_scores_pairwise(const unsigned char *plink, int snps, int indiv, const int *last, double *scores, int adjust) {
  mxa::clear_error();
  if (!last) { mxa::set_error(1, "mxa_ld_window_scores_pairwise: bad arguments"); return 1; }
  return mxa::ld_pairwise_any("mxa_ld_window_scores_pairwise", plink, snps, indiv, 0, last, scores, 0, true, adjust);
}

// ---- the pairs of a window with r^2 >= min_r2 as CSR of the strict upper triangle
extern "C" int mxa_ld_window_pairs(const unsigned char *plink, int snps, int indiv, const int *last, double min_r2, int kind, long *rowptr, int *col, double *val,
                                   long capacity, long *total, int is_plink_format, const double *allele_freq) {
  mxa::clear_error();
  return mxa::ld_pairs_any("mxa_ld_window_pairs", plink, snps, indiv, last, min_r2, kind, rowptr, col, val, capacity, total, false, is_plink_format != 0, allele_freq);
}

extern "C" int mxa_ld_window_pairs_pairwise(const unsigned char *plink, int snps, int indiv, const int *last, double min_r2, int kind, long *rowptr, int *col, double *val,
                                            long capacity, long *total) {
  mxa::clear_error();
  return mxa::ld_pairs_any("mxa_ld_window_pairs_pairwise", plink, snps, indiv, last, min_r2, kind, rowptr, col, val, capacity, total, true, true, nullptr);
}

// ---- the window applied to a matrix: Y = T_w(R) X without the rows
extern "C" int mxa_ld_window_apply(const unsigned char *plink, int snps, int indiv, const int *last, int term, const double *X, long ldx, int n, double *Y, long ldy,
                                   int is_plink_format, const double *allele_freq) {
  mxa::clear_error();
  return mxa::ld_apply_any("mxa_ld_window_apply", plink, snps, indiv, last, term, X, ldx, n, Y, ldy, false, is_plink_format != 0, allele_freq);
}

extern "C" int mxa_ld_window_apply_pairwise(const unsigned char *plink, int snps, int indiv, const int *last, int term, const double *X, long ldx, int n, double *Y,
                                            long ldy) {
  mxa::clear_error();
  return mxa::ld_apply_any("mxa_ld_window_apply_pairwise", plink, snps, indiv, last, term, X, ldx, n, Y, ldy, true, true, nullptr);
}

// The window ends of a distance window, on the host (no device is touched): last[i] = the largest j >= i on i's chromosome with pos[j] - pos[i] <= max_dist
// (one rounded fp64 subtraction, inclusive) and j - i <= max_snps.  All three bounds are monotone in j for fixed i and the end never moves back as i grows,
// so one two-pointer sweep finds every end: O(snps).
extern "C" int mxa_ld_window_bounds(int snps, const double *pos, const int *chrom, double max_dist, int max_snps, int *last, long *rowptr) {
  mxa::clear_error();
  const char *who = "mxa_ld_window_bounds";
  if (snps <= 0 || !last) { mxa::set_error(1, "%s: bad arguments", who); return 1; }
  if (!pos && max_snps < 0) { mxa::set_error(1, "%s: neither a distance bound (pos) nor a SNP bound (max_snps >= 0) is given", who); return 1; }
  if (!(max_dist >= 0.0)) { mxa::set_error(1, "%s: max_dist must not be negative or NaN", who); return 1; }
  if (pos)
    for (long i = 0; i < snps; i++) {
      if (pos[i] != pos[i]) { mxa::set_error(1, "%s: position %ld is NaN", who, i); return 1; }
      if (i > 0 && (!chrom || chrom[i] == chrom[i - 1]) && pos[i] < pos[i - 1]) { mxa::set_error(1, "%s: position %ld decreases inside a chromosome", who, i); return 1; }
    }
  if (chrom) {   // contiguous: a code that starts a run has not been seen before
    std::vector<int> seen;
    for (long i = 0; i < snps; i++)
      if (i == 0 || chrom[i] != chrom[i - 1]) seen.push_back(chrom[i]);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) { mxa::set_error(1, "%s: the SNPs of a chromosome are not contiguous", who); return 1; }
  }
  long j = 0;                                               // the end of the window of i - 1: the window of i reaches at least as far
  for (long i = 0; i < snps; i++) {
    if (j < i) j = i;
    while (j + 1 < snps && (!chrom || chrom[j + 1] == chrom[i]) && (!pos || pos[j + 1] - pos[i] <= max_dist) && (max_snps < 0 || j + 1 - i <= (long)max_snps)) j++;
    last[i] = (int)j;
  }
  if (rowptr) {
    rowptr[0] = 0;
    for (long i = 0; i < snps; i++) rowptr[i + 1] = rowptr[i] + ((long)last[i] - i + 1);
  }
  return 0;
}
