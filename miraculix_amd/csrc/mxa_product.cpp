// mxa_product.cpp -- host driver of the fp64 product C = op(Z) B on one device object: the workspace, the routes of gemm_device (guarded int8, int8 engines,
// column peel, fp64 one-pass and grouped), the host-operand pipeline, and gemm_any / gram_any, which stage operands that are not local to the object's device.
// Everything the library multiplies with -- the C ABI (mxa_api.cpp), the sharded object (mxa_multi.cpp), the association scan (mxa_assoc.hip) -- ends here.
#include "../../include/miraculix_amd.h"
#include "mxa_internal.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

namespace mxa {

// ------------------------------------------------------------------------------------------------ workspace
static int grow(double **p, size_t *cap, size_t need_elems) {
  if (*cap >= need_elems) return 0;
  if (*p) { MXA_HIP(hipFree(*p)); *p = nullptr; *cap = 0; }
  MXA_HIP(hipMalloc(reinterpret_cast<void **>(p), need_elems * sizeof(double)));
  *cap = need_elems;
  return 0;
}

// The partial-sum workspace is sized by ensure_workspace for the plans of n columns; a product that peels odd columns multiplies fewer columns
// with a DIFFERENT plan (tile width, K pieces), which can need more room than the unpeeled one (100 000 x 30 000, n = 9..11: 12.81 M doubles
// against 11.96 M).  Every launch path calls this with the plan it is about to launch.
static int ensure_partials(Workspace &w, const GemmPlan &p, hipStream_t s) {
  const size_t need = (size_t)p.splits * p.n_pad * p.m_pad;
  if (need <= w.cap_P) return 0;
  MXA_HIP(hipStreamSynchronize(s));   // earlier products on this stream may still be reading the old buffer
  return grow(&w.d_P, &w.cap_P, need);
}

// How many doubles of split-K partial sums a product may hold (round 5).  A plan cuts K into pieces whose B slabs stay in an XCD's L2 (plan_gemm), and
// every piece leaves a partial result of the whole output: at BASELINE config 4's full extent (5M SNPs x 200k individuals, n = 128) that is 18 x 5.1 GB
// for 'T' and 407 x 0.2 GB for 'N' beside 250 GB of packed genotypes.  Products whose partials exceed this budget run their K splits in GROUPS
// (gemm_device, "GROUPED K splits"): same pieces, same order of additions, the running sum kept in C.  Budget: everything up to 4 GiB; beyond that at
// most 16 GiB (a group costs one more read + write of C: 18 groups of config 4's 'T' 1.3 % of the call, 6 groups 0.4 %) and at most what the device has
// free right now (the old buffer counted as free: it is released before the new one is allocated) less 2 GiB; never less than ONE split's partials.
// MXA_P_BUDGET_MB overrides (tests force the grouped path on small products).
// The memory-dependent part is decided ONCE per object (Workspace::big_budget, at the first product that needs it): later products reuse it, so a solver
// loop never re-grows the buffer because more memory happens to be free (hipFree + device sync + a multi-GiB hipMalloc in the middle of the loop).
static size_t partial_budget(Workspace &w, size_t need, size_t one_split) {
  const char *e_mb = getenv("MXA_P_BUDGET_MB");   // test knob, read per product: tests/test_grouped_and_incremental_gpu.py switches it on one object
  const long env_mb = e_mb ? atol(e_mb) : -1L;
  if (env_mb >= 0) return std::max(one_split, std::min(need, (size_t)env_mb * (1u << 20) / sizeof(double)));
  if (need * sizeof(double) <= ((size_t)4 << 30) || need <= w.cap_P) return need;
  if (!w.big_budget) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return need; }
    const size_t avail = free_b + w.cap_P * sizeof(double), margin = (size_t)2 << 30, soft = (size_t)16 << 30;
    w.big_budget = std::max<size_t>(1, std::min(soft, avail > margin ? avail - margin : 0) / sizeof(double));
  }
  return std::max(one_split, std::min(need, std::max(w.big_budget, (size_t)w.cap_P)));
}

int ensure_workspace(Handle *h, int n) {
  // sized for the larger of the two products, like the reference's size_buffer (dgemm_compressed_cuda.cu:77)
  Workspace &w = h->ws;
  const long kmax_pad = std::max(h->snp_major.k_pad, h->ind_major.k_pad);
  GemmPlan pn = plan_gemm(h->indiv, h->ind_major.k_pad, n), pt = plan_gemm(h->snps, h->snp_major.k_pad, n);
  const size_t bp = (size_t)kmax_pad * std::max(pn.n_pad, pt.n_pad);
  GemmPlan ln = plan_lut(h->indiv, h->ind_major.k_pad, std::min(n, 4)), lt = plan_lut(h->snps, h->snp_major.k_pad, std::min(n, 4));
  size_t pp = std::max(std::max((size_t)pn.splits * pn.n_pad * pn.m_pad, (size_t)pt.splits * pt.n_pad * pt.m_pad),
                       std::max((size_t)ln.splits * ln.n_pad * ln.m_pad, (size_t)lt.splits * lt.n_pad * lt.m_pad));
  if (grow(&w.d_Bp, &w.cap_Bp, bp)) return 1;
  // very large products keep only a GROUP of their K splits' partial sums at a time (partial_budget, fp64_grouped)
  pp = partial_budget(w, pp, std::max(std::max((size_t)pn.n_pad * pn.m_pad, (size_t)pt.n_pad * pt.m_pad), std::max((size_t)ln.splits * ln.n_pad * ln.m_pad, (size_t)lt.splits * lt.n_pad * lt.m_pad)));
  if (grow(&w.d_P, &w.cap_P, pp)) return 1;
  if (grow(&w.d_colpart, &w.cap_colpart, (size_t)n * (64 * 2 + 2) + 16)) return 1;
  if (!w.d_denflag) {   // flags + the work-queue counters of k_gemm, one small block for the life of the handle
    MXA_HIP(hipMalloc(reinterpret_cast<void **>(&w.d_denflag), (16 + 16 * 16) * sizeof(int)));
    MXA_HIP(hipMemset(w.d_denflag, 0, (16 + 16 * 16) * sizeof(int)));
    w.d_ctr = w.d_denflag + 16;
  }
  return 0;
}

// digits per column of the guarded exact int8 route by column count (guarded_small): class 0 / class 1
static const int kSmallS0[7] = {0, 32, 16, 10, 16, 12, 10}, kSmallS1[7] = {0, 0, 0, 21, 24, 19, 16};

// The int8 workspace the guarded route of an n-column product will ask for (n <= 6: the whole product; n = 4q + r: the r peeled columns), reserved when
// the object is made instead of inside the first product (1.1-1.4 ms of hipMalloc in the first dgemm_compressed call of the reference's harness).
int reserve_small_routes(Handle *h, int n) {
  const int nc = n <= 6 ? n : (n & 3);
  if (nc <= 0 || g_engine.load() != 0) return 0;
  for (int trans = 0; trans < 2; trans++) {
    const PackedMatrix &G = trans ? h->snp_major : h->ind_major;
    if (G.k < 128) continue;
    const PackedMatrix *G_tn = (h->single && !trans) ? &h->snp_major : nullptr;
    if (gemm_i8_reserve(G, nc, kSmallS0[nc], G_tn, h->ws, h->stream) == 1) return 1;
    if (kSmallS1[nc] && gemm_i8_reserve(G, nc, kSmallS1[nc], G_tn, h->ws, h->stream) == 1) return 1;
  }
  return 0;
}

thread_local bool tl_no_warmup = false;   // one-shot objects (dgemm_plink, mxa_assoc_linear) skip the warm-up products
thread_local int tl_centered_override = -1;   // -1: options().centered; 0 / 1: this thread's products are uncentred / centred whatever setOptions_compressed said
static bool product_centered() { return tl_centered_override >= 0 ? tl_centered_override != 0 : options().centered; }
static thread_local bool tl_in_warmup = false;

// First-call costs belong to plink2compressed, not to the first dgemm_compressed (round 6).  The phase clock of the reference's harness showed its FIRST product
// through the plain ABI at 13.5-15.2 ms where the following ones take 4.0 (250k x 50k x 10): 7.2-9.3 ms inside the first device-to-host copy of C on the
// object's stream (the runtime's staged pageable copy; independent of the size, not page faults), 0.8-1.5 ms in the first upload of B, 1.2-1.4 + 0.55 ms of
// first launches of the kernels on the path (profiles/r06_harness_phase_clock.txt).  One 'N' and one 'T' product with max_n columns of zeros, operands where
// the caller's matrices were (host scratch for a host caller: exactly the path its calls will take), pays all of that here -- bounded: the column count
// is cut until a product is estimated below 12.5 ms, and objects whose single-column product is slower than that (HBM-bound at > 60 GB) are not warmed.
// MXA_WARMUP=0 turns it off.  Nothing is timed or counted (timing = false).
int warm_up(Handle *h, bool host_caller) {
  const char *e = getenv("MXA_WARMUP");
  if (tl_no_warmup || (e && atoi(e) == 0)) return 0;
  if (options().centered && !h->has_f) return 0;
  const double cells = (double)h->snps * (double)h->indiv;
  auto est = [&](int nn) { return std::max(2.0 * cells * nn / 70e12, cells / 4.0 / 5e12); };
  int n = h->max_n;
  while (n > 1 && est(n) > 0.0125) n = n > 8 ? (n / 2 + 3) / 4 * 4 : n - 1;
  if (est(n) > 0.0125) return 0;
  const size_t cnt = (size_t)std::max(h->snps, h->indiv) * n;
  int rc = 0;
  tl_in_warmup = true;
  if (host_caller) {
    double *hb = (double *)calloc(cnt, sizeof(double)), *hc = (double *)malloc(cnt * sizeof(double));
    if (hb && hc) {
      rc = gemm_any(h, false, n, hb, h->snps, hc, h->indiv, h->indiv, true, false);
      if (!rc) rc = gemm_any(h, true, n, hb, h->indiv, hc, h->snps, h->snps, true, false);
    }
    free(hb); free(hc);
  } else {
    Workspace &w = h->ws;
    if (grow(&w.d_Bstage, &w.cap_Bstage, cnt) || grow(&w.d_Cstage, &w.cap_Cstage, cnt)) { tl_in_warmup = false; return 1; }
    if (!check_hip(hipMemsetAsync(w.d_Bstage, 0, cnt * sizeof(double), h->stream), __func__, __LINE__)) { tl_in_warmup = false; return 1; }
    rc = gemm_device(h, false, n, w.d_Bstage, h->snps, w.d_Cstage, h->indiv, h->indiv, h->stream, false);
    if (!rc) rc = gemm_device(h, true, n, w.d_Bstage, h->indiv, w.d_Cstage, h->snps, h->snps, h->stream, false);
    if (!rc && !check_hip(hipStreamSynchronize(h->stream), __func__, __LINE__)) rc = 1;
  }
  { std::lock_guard<std::mutex> lk(g_prof_mutex); last_geometry() = Geometry(); }   // mxa_last_path / mxa_last_geometry describe the CALLER'S products
  harvest_profile(h);
  h->prof = ObjectProfile();            // ... and so do the per-object counters
  tl_in_warmup = false;
  return rc;
}


// Column-major block copy (height columns of `width` bytes, pitches in bytes) between host / device memory: one hipMemcpy2DAsync (a strided
// 100 MB download takes 1.8 ms this way and 7.7 ms as one 1-D copy per column).  Exception: strided DOWNLOADS issued by the shard worker
// threads of a multi-device object go column by column.  hipMemcpy2DAsync to pageable host memory issued from several threads at the same
// time leaves device memory behind on ROCm 7.2 (0.2-0.6 MiB per shard and object life cycle; not with HIP_LAUNCH_BLOCKING=1, not from a
// single thread, not with 1-D copies: tools/soak_lifecycle.py), and a long-lived session must not creep.
static thread_local bool tl_concurrent = false;
void mark_thread_concurrent() { tl_concurrent = true; }
static hipError_t copy_columns(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipStream_t s) {
  if (width == 0 || height == 0) return hipSuccess;
  if (dpitch == width && spitch == width) return hipMemcpyAsync(dst, src, width * height, hipMemcpyDefault, s);
  if (height == 1) return hipMemcpyAsync(dst, src, width, hipMemcpyDefault, s);
  const bool per_column = tl_concurrent && ptr_location(dst, nullptr) == 0;
  if (!per_column) return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDefault, s);
  for (size_t j = 0; j < height; j++) {
    const hipError_t e = hipMemcpyAsync(static_cast<char *>(dst) + j * dpitch, static_cast<const char *>(src) + j * spitch, width, hipMemcpyDefault, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ------------------------------------------------------------------------------------------------ multiply
static bool elapsed_ms(hipEvent_t a, hipEvent_t b, float *ms) {
  if (hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(ms, a, b) != hipSuccess) { (void)hipGetLastError(); return false; }
  return true;
}
static void harvest_slot(Handle *h, int slot) {
  if (!h->prof_pending[slot]) return;
  h->prof_pending[slot] = false;
  float ms = 0.f;
  if (!elapsed_ms(h->ev0[slot], h->ev1[slot], &ms)) return;
  std::lock_guard<std::mutex> lk(g_prof_mutex);
  profile().launches += 1; profile().total_ms += ms;
  h->prof.launches += 1; h->prof.kernel_ms += ms;
  h->prof_last_kernel_ms = ms;
}
static void harvest_copies(Handle *h) {
  float ms = 0.f;
  if (h->in_pending) { h->in_pending = false; if (elapsed_ms(h->ev_in[0], h->ev_in[1], &ms)) { h->prof.in_copies += 1; h->prof.in_ms += ms; h->prof_last_in_ms = ms; } }
  if (h->out_pending) { h->out_pending = false; if (elapsed_ms(h->ev_out[0], h->ev_out[1], &ms)) { h->prof.out_copies += 1; h->prof.out_ms += ms; h->prof_last_out_ms = ms; } }
}
void harvest_profile(Handle *h) {
  if (!h) return;
  harvest_slot(h, 0); harvest_slot(h, 1);
  harvest_copies(h);
}

int sync_foreign_producer(int src_dev) {
  int cur = 0;
  MXA_HIP(hipGetDevice(&cur));
  if (src_dev < 0 || src_dev == cur) return 0;
  MXA_HIP(hipSetDevice(src_dev));
  const hipError_t e = hipStreamSynchronize(nullptr);
  MXA_HIP(hipSetDevice(cur));
  MXA_HIP(e);
  return 0;
}

int enable_peer(int cur, int peer) {
  if (cur == peer) return 1;
  int prev = 0, can = 0;
  if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); return 0; }
  if (hipSetDevice(cur) != hipSuccess) { (void)hipGetLastError(); return 0; }
  if (hipDeviceCanAccessPeer(&can, cur, peer) != hipSuccess) { (void)hipGetLastError(); can = 0; }
  if (can) {
    const hipError_t e = hipDeviceEnablePeerAccess(peer, 0);
    if (e != hipSuccess) (void)hipGetLastError();
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) can = 0;
  }
  (void)hipSetDevice(prev);
  return can;
}

// Which stored orientation feeds a k_gemm launch (round 4).  Every product can be computed from either copy: in the plain form from the copy whose ROWS
// are the output rows ('T': SNP-major, 'N': individual-major -- the reference's choice, dgemm_compressed_cuda.cu:270), in the transposed-operand form
// (k_gemm<..., TR>) from the copy whose rows are the K index.  The two forms give bit-identical results (same plan, same K order).  The transposed form
// reads the genotype operand with ONE LDS instruction per K-step instead of A / 2 and extracts every fragment with a two-operand v_and_b32 whose scale
// belongs to the output row (undone exactly in the epilogue), for every tile.  Measured, same box, alternating (profiles/r04_gemm_tr_ab.txt): C2
// 42.5 ms per launch against 43.9-44.0 = 75.3 against 72.8 TFLOP/s = 0.957 against 0.925 of the fp64 MFMA peak; config-4 shard 423.6 against 438.0 ms
// (0.961); n = 20: 13.55 against 13.98; n = 16: 10.87 against 11.03; n = 12: 8.30-8.35 against 8.44-8.47; n = 8: 5.70 against 5.77-5.84.
// MXA_GEMM_TR: 0 never (the plain form), otherwise / unset: always.  Read per call.
static bool gemm_use_tr(const GemmPlan &, const Handle *h, bool trans) {
  if (h->single) return !trans;            // one stored copy (SNP-major): 'N' transposed, 'T' plain
  const char *e = getenv("MXA_GEMM_TR");
  return !e || atoi(e) != 0;
}
static const PackedMatrix &gemm_operand(const Handle *h, bool trans, bool tr) { return (trans != tr) ? h->snp_major : h->ind_major; }

constexpr int kSmallNMaxColsHost = 6;   // widest product that takes the guarded exact int8 route whole (mxa_gemm_i8.hip: kSmallNMaxCols)

// One product as gemm_device sees it; built once per call and handed to the routes below.
struct Product {
  Handle *h; Workspace &w;
  const PackedMatrix &G;          // the copy whose rows are the output rows; the reference picks d_plink for 'T' (dgemm_compressed_cuda.cu:270)
  bool trans, centered;
  long m, k;
  int n;                          // columns still to multiply (the peel takes the odd ones off the end)
  const double *dB; long ldb;
  double *dC; long ldc, fill_rows;
  double *d_sumB, *d_sumfB;       // column sums of the centring term, n each
  hipStream_t s;
  // Single-orientation object, 'N': the plain int8 kernel needs the individual-major copy; k_gemm_i8_tn multiplies from the SNP-major one (G_tn_single), one
  // pass per tile of 32 expanded columns; a class whose passes would cost more than the fp64 MFMA tile is not offered (gemm_i8_reserve returns 2).
  bool no_plain; const PackedMatrix *G_tn_single;
  bool prof; int slot; hipEvent_t pe0, pe1;   // timing: the event pair around the dominant kernel (nullptr when off)
};

// what mxa_last_path / mxa_last_geometry report; d_flag: the device word that settles path 4 (read by mxa_last_path, never for another path)
static void record_geometry(const Handle *h, long m, long k, int n, int splits, int a, int c, int path, const int *d_flag = nullptr) {
  std::lock_guard<std::mutex> lk(g_prof_mutex);
  Geometry &geo = last_geometry();
  geo.m = m; geo.k = k; geo.n = n; geo.splits = splits; geo.a = a; geo.c = c; geo.path = path; geo.d_flag = d_flag; geo.flag_dev = h->device;
}

// room for `count` per-column exponents of B (denormal-operand mode)
static int ensure_exponents(Workspace &w, size_t count, hipStream_t s) {
  if (w.cap_exp >= count) return 0;
  MXA_HIP(hipStreamSynchronize(s));
  if (w.d_exp) { MXA_HIP(hipFree(w.d_exp)); w.d_exp = nullptr; w.cap_exp = 0; }
  MXA_HIP(hipMalloc(reinterpret_cast<void **>(&w.d_exp), sizeof(int) * count));
  w.cap_exp = count;
  return 0;
}

// the argument checks of a product, shared by gemm_device and gemm_host_pipelined (gemm_any: the leading dimensions, ahead of the centring that gemm_device checks)
static int check_product(const Handle *h, bool centered, long ldb, long k, long ldc, long m) {
  if (centered && !h->has_f) { set_error(6, "dgemm_compressed: centring requested but no allele frequencies were supplied to plink2compressed"); return 1; }
  if (ldb < k || ldc < m) { set_error(7, "dgemm_compressed: leading dimension too small (ldb %ld < %ld or ldc %ld < %ld)", ldb, k, ldc, m); return 1; }
  return 0;
}

// ---- the guarded exact int8 route of narrow products and of peeled columns (HBM-bound).
// B is split exactly into balanced radix-256 digits and multiplied on the int8 matrix cores with exact integer sums WHEN THAT IS EXACT: every column
// finite, its exponent span within the digits (e_max - e_min <= 8 S - 55), no underflow in the recombination.  Then no bit of B is dropped and the
// only roundings are the S - 1 additions of the recombination: |error| <= 3.02 (S - 1) 2^-53 sum_k |z_k b_k|, below the K 2^-53 sum |z b| of an fp64
// chain for K >= 128.  The verdict is formed ON THE DEVICE (round 5: for every n, not only n <= 2) as a class -- class 0: exact with the digits of the
// cheapest tile count, class 1: exact with one more tile of digits, class 2: not exact -- and the chains of both classes plus the fp64 kernel behind
// them are all enqueued, each testing one flag word: NO product waits for the host (rounds 3-4 read three integers back for 3 <= n <= 6 and peeled
// columns).  Digits per column by n: what fits the tiles of 32 expanded columns -- n = 1: 32; 2: 16; 3: 10 | 21; 4: 16 | 24; 5: 12 | 19; 6: 10 | 16.
// columns [c0, c0 + nc), nc <= 6.  0: enqueued (int8 chains + fp64 kernel: the columns are done whatever the verdict), 2: not applicable, 1: error
// Verdict class 2 ("not exactly representable"; inf / NaN; a column near the underflow threshold): who does the product in fp64?
//   nc = 1: fp64 chains, one thread per output row, inside the first chain's k_slice_B launch (no launch of their own: the CG step counts its launches; with 32 digits =
//           201 binades the class needs inf / NaN or an entry 60 decades below its column's maximum).
//   nc >= 2: the plain-operand fp64 path behind the chains, every launch gated by the verdict word -- k_lut + k_finish (nc = 2, plain form) or k_pack_B + k_gemm<MODE 0>
//           + k_finish: three empty launches (~5 us each) on a >= 1 ms product when the int8 classes apply, against 45-280 ms of chains when they do not
//           (500k x 50k, n = 4 .. 6: measured late in round 5).  If its partial sums do not fit the budget (objects that fill the device): the chains.
// timed: the first chain is bracketed by the product's event pair; splits_out / flag_ptr nullable.
static int guarded_small(const Product &pr, int c0, int nc, const PackedMatrix *G_tn, bool timed, int *splits_out, const int **flag_ptr) {
  Handle *h = pr.h; Workspace &w = pr.w; const PackedMatrix &G = pr.G; hipStream_t s = pr.s;
  I8Chain ch; ch.S0 = kSmallS0[nc]; ch.S1 = kSmallS1[nc];
  const bool fb_lut = nc <= 2 && !pr.no_plain;
  GemmPlan pf = fb_lut ? plan_lut(pr.m, G.k_pad, nc) : plan_gemm(pr.m, G.k_pad, nc);
  bool fast_fb = nc >= 2;
  if (fast_fb) {
    const size_t one = (size_t)pf.n_pad * pf.m_pad, need = one * pf.splits;
    fast_fb = partial_budget(w, need, one) >= need;
  }
  ch.fp64_rows = !fast_fb;
  const int r0 = gemm_i8_reserve(G, nc, ch.S0, G_tn, w, s);
  if (r0) return r0;
  if (ch.S1) {
    const int r1 = gemm_i8_reserve(G, nc, ch.S1, G_tn, w, s);
    if (r1 == 1) return 1;
    if (r1 == 2) ch.S1 = 0;   // the larger class is not offered (transposed form: more passes than the fp64 kernel is worth)
  }
  const double *dBc = pr.dB + (size_t)c0 * pr.ldb;
  double *dCc = pr.dC + (size_t)c0 * pr.ldc;
  double *d_sumB = pr.d_sumB + c0, *d_sumfB = pr.d_sumfB + c0;
  const int *d_flag = nullptr;
  for (int cls = 0; cls < (ch.S1 ? 2 : 1); cls++) {
    ch.my_class = cls; ch.first = cls == 0;
    const bool lead = cls == 0;
    const I8Opts o = {.ev0 = lead && timed ? pr.pe0 : nullptr, .ev1 = lead && timed ? pr.pe1 : nullptr, .splits_out = lead ? splits_out : nullptr, .flag_out = &d_flag, .colsum_scratch = w.d_colpart, .G_tn = G_tn, .chain = &ch};
    const int rc = gemm_i8_device(G, pr.trans, nc, dBc, pr.ldb, dCc, pr.ldc, pr.fill_rows, pr.centered, d_sumB, d_sumfB, h->d_f, w, s, o);
    if (rc != 3) return 1;
  }
  if (fast_fb) {   // class 2: the gated fp64 launches (d_flag = the word "class == 2")
    if (ensure_partials(w, pf, s)) return 1;
    if (fb_lut) { if (launch_lut(G, dBc, pr.ldb, nc, w.d_P, pf, s, d_flag)) return 1; }
    else {
      const bool trf = gemm_use_tr(pf, h, pr.trans);
      if (launch_pack_B(dBc, pr.ldb, pr.k, nc, w.d_Bp, G.k_pad, pf.n_pad, pf.c, s, {.run_if_set = d_flag})) return 1;
      if (launch_gemm(gemm_operand(h, pr.trans, trf), w.d_Bp, w.d_P, pf, 0, s, next_ctr(w), {.run_if_set = d_flag, .tr = trf})) return 1;
    }
    if (launch_finish(w.d_P, pf, pr.m, nc, dCc, pr.ldc, pr.fill_rows, pr.trans ? 1 : 0, pr.centered, d_sumB, d_sumfB, h->d_f, s, {.run_if_set = d_flag})) return 1;
  }
  // (class 2 at nc = 1: plain fp64 chains, one thread per output row, inside the first chain's k_slice_B launch)
  if (flag_ptr) *flag_ptr = d_flag;
  return 0;
}

// a whole product of n <= 6 columns through the guarded route.  0 done, 1 error, 2 not applicable
static int guarded_product(const Product &pr) {
  const char *e_tn = getenv("MXA_I8_TN");   // A/B (read per call): n <= 2 from the copy whose rows are the K index
  const bool tn_ab = e_tn && atoi(e_tn) != 0;
  const PackedMatrix *G_tn = pr.no_plain ? pr.G_tn_single : (tn_ab && pr.n <= 2 && !pr.h->single) ? &gemm_operand(pr.h, pr.trans, true) : nullptr;   // (the A/B needs both stored copies)
  int splits8 = 1;
  const int *d_flag = nullptr;
  const int rc = guarded_small(pr, 0, pr.n, G_tn, true, &splits8, &d_flag);
  if (rc) return rc;
  // (the range flag of the denormal-operand mode -- mxa_last_range_fallback -- is cleared by the chain's k_slice_B)
  record_geometry(pr.h, pr.m, pr.k, pr.n, splits8, 0, 0, 4, d_flag);
  pr.h->prof_pending[pr.slot] = pr.prof;
  return 0;
}

// Engines 1 / 4 (opt-in): the int8 slicing of all n columns with S digits each (0: plan_i8's choice).  Plain form: one call.  Transposed-operand form ('N' of a
// one-copy object): k_gemm_i8_tn takes at most six tiles of 32 expanded columns per call (three passes of two tiles), so a wide product goes in balanced column
// chunks -- every pass streams the packed matrix once, and three columns' worth of fp64 MFMA time buys a pass (C2, n = 32, 10 digits: 6 passes of 2.9 ms against
// 43 ms on the fp64 tile).  stats_base: column maxima that are already there (k_colmax_partial's layout: the maxima of column j at [64 j, 64 j + 64)).
// 0 done, 1 error, 2 declined with nothing enqueued
static int i8_engine_product(const Product &pr, int S, double *stats_base, int *splits_out) {
  Handle *h = pr.h; const int n = pr.n;
  const int rc = gemm_i8_device(pr.G, pr.trans, n, pr.dB, pr.ldb, pr.dC, pr.ldc, pr.fill_rows, pr.centered, pr.d_sumB, pr.d_sumfB, h->d_f, pr.w, pr.s,
                                {.ev0 = pr.pe0, .ev1 = pr.pe1, .splits_out = splits_out, .S_override = S, .G_tn = pr.G_tn_single, .stats_part = stats_base});
  if (rc != 2 || !pr.G_tn_single) return rc;
  const int cmax = (6 * 32) / (S > 0 ? S : 7);
  if (cmax < 1) return 2;
  const int chunks = (n + cmax - 1) / cmax, per = (n + chunks - 1) / chunks;
  if (chunks < 2) return 2;                  // declined for another reason than the tile count (K beyond the accumulators' range)
  for (int c0 = 0; c0 < n; c0 += per) {
    const int nc = std::min(per, n - c0);
    const I8Opts o = {.ev0 = c0 == 0 ? pr.pe0 : nullptr, .ev1 = c0 + nc >= n ? pr.pe1 : nullptr, .splits_out = splits_out, .S_override = S, .G_tn = pr.G_tn_single, .stats_part = stats_base ? stats_base + (size_t)c0 * 64 : nullptr};
    const int rcc = gemm_i8_device(pr.G, pr.trans, nc, pr.dB + (size_t)c0 * pr.ldb, pr.ldb, pr.dC + (size_t)c0 * pr.ldc, pr.ldc, pr.fill_rows, pr.centered, pr.d_sumB + c0, pr.d_sumfB + c0, h->d_f, pr.w, pr.s, o);
    if (rcc == 2 && c0 == 0) return 2;       // nothing is enqueued yet: the fp64 path takes the product
    if (rcc) { if (rcc == 2) set_error(4, "internal: a later column chunk of the int8 engine declined"); return 1; }
  }
  return 0;
}

// The opt-in int8 engines on a whole product.  Engine 1: the slicing without the exactness check (7 digits; 32 / 16 for n = 1 / 2).  Engine 4 (i8-exact): the
// same exact slicing for EVERY n with the digit count chosen PER CALL from the measured exponent span of B's columns -- S = max(7, ceil((span + 55) / 8)) <= 24
// -- by the host: three integers are read back (ONE host synchronisation per call, documented with the engine).
// 0 done, 1 error, 2 the fp64 path takes the product: the span wants more digits than engine 4 has, or the int8 route declined (K beyond the accumulators' range
// in the transposed-operand form)
static int i8_engine_route(const Product &pr, int engine) {
  Workspace &w = pr.w; hipStream_t s = pr.s;
  int splits8 = 1, S = 0, hs[3] = {0, 0, 1};
  if (engine == 4) {
    if (launch_colspan(pr.dB, pr.ldb, pr.k, pr.n, w.d_colpart, w.d_denflag + 4, s)) return 1;
    MXA_HIP(hipMemcpyAsync(hs, w.d_denflag + 4, sizeof(hs), hipMemcpyDeviceToHost, s));
    MXA_HIP(hipStreamSynchronize(s));
    S = std::max(7, (hs[0] + 55 + 7) / 8);
    if (hs[2] || S > kI8ExactMaxDigits || hs[1] < 8 * S - 1023) return 2;
  }
  const int rc = i8_engine_product(pr, S, engine == 4 ? w.d_colpart : nullptr, &splits8);
  if (rc) return rc == 2 ? 2 : 1;
  if (engine == 4) MXA_HIP(hipMemsetAsync(w.d_denflag, 0, sizeof(int), s));
  record_geometry(pr.h, pr.m, pr.k, pr.n, splits8, S, 0, 2);
  pr.h->prof_pending[pr.slot] = pr.prof;
  return 0;
}

// the rest of a product after the routes above: the fp64 MFMA tile (or the pair tables: n <= 2 of engine f64-strict and of K < 128)
// splits_per_group: K splits per launch group, all of them unless their partial sums exceed the budget (partial_budget); tr: transposed-operand form, from the
// OTHER stored orientation (gemm_use_tr); GL: the stored copy that feeds k_gemm; mode 2 / 3 (default): genotype operand as the denormal z * 2^-1074 (one VALU
// per fragment instead of two), B scaled per column by the exponents d_E (nullptr: MODE 0, pair tables)
struct Fp64Launch { GemmPlan p; bool use_lut, tr; int splits_per_group, mode; const PackedMatrix *GL; const int *d_E; };

// One pass: pack, gemm, the gated plain-operand pack + gemm behind them (fallback of the denormal-operand mode, run only when the guard raised the flag:
// unscaled B, two-instruction conversion), one finish.
static int fp64_one_pass(const Product &pr, const Fp64Launch &f) {
  Handle *h = pr.h; Workspace &w = pr.w; hipStream_t s = pr.s;
  const GemmPlan &p = f.p;
  int rc = f.use_lut ? launch_lut(pr.G, pr.dB, pr.ldb, pr.n, w.d_P, p, s) : launch_gemm(*f.GL, w.d_Bp, w.d_P, p, f.mode, s, next_ctr(w), {.tr = f.tr});
  if (pr.prof && !rc) { MXA_HIP(hipEventRecord(pr.pe1, s)); h->prof_pending[pr.slot] = true; }
  if (!rc && f.d_E) {
    rc = launch_pack_B(pr.dB, pr.ldb, pr.k, pr.n, w.d_Bp, pr.G.k_pad, p.n_pad, p.c, s, {.run_if_set = w.d_denflag});
    if (!rc) rc = launch_gemm(*f.GL, w.d_Bp, w.d_P, p, 0, s, next_ctr(w), {.run_if_set = w.d_denflag, .tr = f.tr});
  }
  if (!rc) rc = launch_finish(w.d_P, p, pr.m, pr.n, pr.dC, pr.ldc, pr.fill_rows, pr.trans ? 1 : 0, pr.centered, pr.d_sumB, pr.d_sumfB, h->d_f, s, {.d_E = f.d_E, .unscaled_if_set = f.d_E ? w.d_denflag : nullptr});
  return rc;
}

// GROUPED K splits (round 5; BASELINE config 4 at its full 5M x 200k x 128 on one device): the launch plan is unchanged -- same pieces, same K
// order -- but only `splits_per_group` splits are in flight at a time; each group's partial sums are added to the running sum kept in C (raw: no
// scale-back, no centring) and the last group applies the epilogue.  One sequential ascending chain of additions, as in the one-pass k_finish:
// bit-identical to it (tests/test_grouped_and_incremental_gpu.py).  Pass 1 = the plain-operand fallback of the denormal-operand mode, gated by the
// range flag like the one-pass path: it redoes every group and overwrites C.
static int fp64_grouped(const Product &pr, const Fp64Launch &f) {
  Handle *h = pr.h; Workspace &w = pr.w; hipStream_t s = pr.s;
  const GemmPlan &p = f.p;
  const size_t stride = (size_t)p.n_pad * p.m_pad;
  for (int pass = 0; pass < (f.d_E ? 2 : 1); pass++) {
    const int *gate = pass ? w.d_denflag : nullptr;
    if (pass && launch_pack_B(pr.dB, pr.ldb, pr.k, pr.n, w.d_Bp, pr.G.k_pad, p.n_pad, p.c, s, {.run_if_set = gate})) return 1;
    for (int sb = 0; sb < p.splits; sb += f.splits_per_group) {
      const int se = std::min(p.splits, sb + f.splits_per_group);
      // split sb lands at the start of the buffer (p_split0 = sb)
      if ((size_t)(se - sb) * stride > w.cap_P) { set_error(4, "internal: a group of %d K splits exceeds the partial-sum workspace", se - sb); return 1; }
      if (launch_gemm(*f.GL, w.d_Bp, w.d_P, p, pass ? 0 : f.mode, s, next_ctr(w), {.split_begin = sb, .split_end = se, .run_if_set = gate, .tr = f.tr, .p_split0 = sb})) return 1;
      const FinishOpts o = {.d_E = pass ? nullptr : f.d_E, .run_if_set = gate, .group_splits = se - sb, .group = (sb > 0 ? 1 : 0) | (se < p.splits ? 2 : 0)};
      if (launch_finish(w.d_P, p, pr.m, pr.n, pr.dC, pr.ldc, pr.fill_rows, pr.trans ? 1 : 0, pr.centered, pr.d_sumB, pr.d_sumfB, h->d_f, s, o)) return 1;
    }
    if (!pass && pr.prof) { MXA_HIP(hipEventRecord(pr.pe1, s)); h->prof_pending[pr.slot] = true; }
  }
  return 0;
}

// plan, partial sums, geometry, exponents + range guard and the packed B of pr.n columns; then one pass or the groups
static int fp64_product(const Product &pr) {
  Handle *h = pr.h; Workspace &w = pr.w; const PackedMatrix &G = pr.G; hipStream_t s = pr.s;
  const int n = pr.n;
  Fp64Launch f;
  f.use_lut = n <= 2 && !pr.no_plain;   // fp64 pair tables: engine f64-strict, and K < 128
  f.p = f.use_lut ? plan_lut(pr.m, G.k_pad, n) : plan_gemm(pr.m, G.k_pad, n);
  const GemmPlan &p = f.p;
  f.splits_per_group = p.splits;
  if (!f.use_lut) {
    const size_t one = (size_t)p.n_pad * p.m_pad, need = one * p.splits;
    const size_t budget = partial_budget(w, need, one);
    if (budget < need) {
      f.splits_per_group = (int)std::max<size_t>(1, budget / one);
      GemmPlan pg = p; pg.splits = f.splits_per_group;
      if (ensure_partials(w, pg, s)) return 1;
    }
  }
  if (f.splits_per_group == p.splits && ensure_partials(w, p, s)) return 1;   // the plan of the columns left after a peel may need more than the plan ensure_workspace sized for
  clock_mark("partials");
  record_geometry(pr.h, pr.m, pr.k, n, p.splits, p.a, p.c, f.use_lut ? 1 : 0);
  f.tr = !f.use_lut && gemm_use_tr(p, h, pr.trans);
  f.GL = &gemm_operand(h, pr.trans, f.tr);
  f.mode = gemm_default_mode(p.c);
  f.d_E = nullptr;
  if (!f.use_lut && (f.mode == 2 || f.mode == 3)) {
    if (ensure_exponents(w, (size_t)n, s)) return 1;
    // per-column exponents + the range guard of the mode: a column whose non-zero entries span more than kDenMaxSpan binades (or that
    // holds inf / NaN) raises d_denflag, and the plain-operand chain redoes the product (the verdict stays on the device)
    if (launch_colexp(pr.dB, pr.ldb, pr.k, n, w.d_colpart, w.d_exp, 0, s, w.d_denflag, kDenMaxSpan, -100000)) return 1;
    f.d_E = w.d_exp;
  }
  if (!f.use_lut && launch_pack_B(pr.dB, pr.ldb, pr.k, n, w.d_Bp, G.k_pad, p.n_pad, p.c, s, {.d_E = f.d_E, .rowscale = f.mode == 3 && !f.tr})) return 1;
  if (pr.prof) MXA_HIP(hipEventRecord(pr.pe0, s));
  return f.splits_per_group < p.splits ? fp64_grouped(pr, f) : fp64_one_pass(pr, f);
}

// Device operands only; asynchronous on s.  With timing, ev0/ev1 bracket the dominant kernel and harvest_profile() reads them later.
int gemm_device(Handle *h, bool trans, int n, const double *dB, long ldb, double *dC, long ldc, long fill_rows, hipStream_t s, bool timing) {
  const PackedMatrix &G = trans ? h->snp_major : h->ind_major;
  const long m = G.rows, k = G.k;
  const bool centered = product_centered();
  if (check_product(h, centered, ldb, k, ldc, m)) return 1;
  if (fill_rows < m || fill_rows > ldc) { set_error(7, "internal: fill_rows %ld outside [%ld, %ld]", fill_rows, m, ldc); return 1; }
  if (n > 65535) { set_error(7, "dgemm_compressed: n = %d exceeds the supported 65535 columns per call", n); return 1; }
  if (n > h->max_n) { h->max_n = n; }
  if (ensure_workspace(h, n)) return 1;
  clock_mark("workspace");
  Workspace &w = h->ws;
  const bool no_plain = h->single && !trans;
  Product pr = {h, w, G, trans, centered, m, k, n, dB, ldb, dC, ldc, fill_rows, w.d_colpart + (size_t)n * 128, w.d_colpart + (size_t)n * 128 + n, s,
                no_plain, no_plain ? &gemm_operand(h, trans, true) : nullptr, g_profile_on && timing, h->prof_slot, nullptr, nullptr};
  if (pr.prof) {
    if (!h->ev0[pr.slot]) { MXA_HIP(hipEventCreate(&h->ev0[pr.slot])); MXA_HIP(hipEventCreate(&h->ev1[pr.slot])); }
    harvest_slot(h, pr.slot);   // the pair of the product before last is read before it is recorded again
    h->prof_slot = pr.slot ^ 1;
    clock_mark("prof-events");
    pr.pe0 = h->ev0[pr.slot]; pr.pe1 = h->ev1[pr.slot];
  }
  const int engine = g_engine.load();
  const bool small_ok = (engine == 0 || (engine == 4 && n <= 2)) && k >= 128;
  int rc = 2;   // 2: the route does not apply or declined with nothing enqueued -- the next one takes the product
  if (small_ok && n <= kSmallNMaxColsHost && (rc = guarded_product(pr)) != 2) return rc;
  if (centered && launch_colsums(dB, ldb, k, n, trans ? nullptr : h->d_f, w.d_colpart, pr.d_sumB, pr.d_sumfB, s)) return 1;
  if (((engine == 4 && k >= 128 && n > 2) || engine == 1) && (rc = i8_engine_route(pr, engine)) != 2) return rc;
  // Column peel (engine 0, n = 4q + r > 6, r = 1, 2, 3): the MFMA tile works on groups of 4 columns, so 10 columns would cost 12 (the reference harness's
  // default n = 10).  The r odd columns go through the guarded route -- one HBM-bound pass over the packed matrix -- and the multiple of 4 runs on the
  // fp64 MFMA without padding.
  const int n_odd = n & 3;
  if (small_ok && n > kSmallNMaxColsHost && n_odd != 0) {
    const int rcp = guarded_small(pr, n - n_odd, n_odd, pr.G_tn_single, false, nullptr, nullptr);
    if (rcp == 1) return 1;
    if (rcp == 0) pr.n -= n_odd;         // fp64_product multiplies the first 4q columns
    clock_mark("peel-enqueued");
  }
  return fp64_product(pr);
}


// ------------------------------------------------------------------------------------------------ host-operand pipeline
// The plain reference ABI hands over HOST B and C (utils/benchmark/benchmark.f90:192-209 times exactly that).  At C2 a call moves 269 MB over
// PCIe (5.4 ms at the ~50 GB/s a pageable copy reaches) around a 44 ms product.  Both transfers are hidden behind the product:
//   big B (K-chunk mode, 'N'): the K splits of the launch plan are cut into <= 8 groups; group c's rows of B are uploaded (the host
//     thread blocks in the staged pageable copy while the GPU multiplies group c-1), scaled and packed on their own (per-group column
//     exponents), and multiplied by a launch over just those splits.  Groups alternate between two streams so that the ramp of one launch
//     fills the drain of the previous one.  One k_finish adds all partials in the usual ascending order, each scaled back by its group's
//     exponent first -- power-of-two scaling commutes with rounding, so the result is bit-identical to the one-launch path.
//   big C (M-chunk mode, 'T'): B is uploaded and packed once; <= 8 row ranges of the packed matrix are multiplied and finished by launches of
//     their own (same split count as the one-launch plan, so identical sums), alternating between the two streams, and every finished row
//     range travels to the host while the next one is computed.
constexpr int kPipeChunks = 8;            // at most; at least ~8 MB of transfer per chunk
static const size_t kPipeMinBytes = (size_t)32 << 20;

static int pipe_setup(Handle *h) {
  for (hipStream_t &ps : h->pipe) if (!ps) MXA_HIP(hipStreamCreateWithFlags(&ps, hipStreamNonBlocking));
  for (hipEvent_t &e : h->pev) if (!e) MXA_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return 0;
}

// returns 0 done, 1 error, 2 not applicable (caller takes the plain path)
static int gemm_host_pipelined(Handle *h, bool trans, int n, const double *B, long ldb, bool b_host, bool b_local, double *C, long ldc, bool c_host, bool c_local,
                               long fill_rows) {
  const int engine = g_engine.load();
  if ((engine != 0 && engine != 3) || n < 3 || getenv("MXA_DIAG")) return 2;
  if (engine == 0 && n <= kSmallNMaxColsHost) return 2;   // engine 0 sends n <= 6 through the guarded int8 route of gemm_device (plain upload; B is at most 6 columns)
  const PackedMatrix &G = trans ? h->snp_major : h->ind_major;
  const long m = G.rows, k = G.k;
  // b_host / c_host: the operand is not memory of this device -- host memory (PCIe) or memory of another GPU (peer copies over xGMI):
  // either way its transfer is hidden behind the product
  const size_t b_bytes = b_host ? sizeof(double) * (size_t)k * n : 0, c_bytes = c_host ? sizeof(double) * (size_t)m * n : 0;
  if (std::max(b_bytes, c_bytes) < kPipeMinBytes) return 2;
  const bool kmode = b_bytes >= c_bytes;
  const bool centered = product_centered();
  if (check_product(h, centered, ldb, k, ldc, m)) return 1;
  if (n > h->max_n) h->max_n = n;
  if (ensure_workspace(h, n) || pipe_setup(h)) return 1;
  harvest_profile(h);
  Workspace &w = h->ws;
  hipStream_t s = h->stream;
  // scratch: per-group column-maximum partials (64 n doubles each) + column sums; per-group exponents
  if (grow(&w.d_colpart, &w.cap_colpart, (size_t)n * (128 * (kPipeChunks + 1) + 2) + 16)) return 1;
  if (ensure_exponents(w, (size_t)n * kPipeChunks, s)) return 1;
  double *d_sumB = w.d_colpart + (size_t)n * 128 * (kPipeChunks + 1), *d_sumfB = d_sumB + n;
  double *d_sumscratch = w.d_colpart + (size_t)n * 128 * kPipeChunks;   // 128 n doubles for launch_colsums
  // operands on this device
  const double *dB = B; long dldb = ldb;
  if (!b_local) { if (grow(&w.d_Bstage, &w.cap_Bstage, (size_t)k * n)) return 1; dB = w.d_Bstage; dldb = k; }
  double *dC = C; long dldc = ldc;
  if (!c_local) { if (grow(&w.d_Cstage, &w.cap_Cstage, (size_t)fill_rows * n)) return 1; dC = w.d_Cstage; dldc = fill_rows; }
  // column peel as in gemm_device: the 1-3 odd columns go first (their part of B is uploaded ahead of the pipeline) through the same guarded exact int8
  // route -- gemm_device itself on those columns, so that the host path stays bitwise the device path --; the K-range / row-range pipeline then multiplies
  // the multiple of 4
  const int n_all = n, n_odd = n & 3;
  bool b_uploaded = false;
  if (engine == 0 && n > kSmallNMaxColsHost && n_odd != 0 && k >= 128) {
    const int n4 = n - n_odd;
    if (!b_local) {
      if (kmode) MXA_HIP(copy_columns(w.d_Bstage + (size_t)n4 * k, sizeof(double) * k, B + (size_t)n4 * ldb, sizeof(double) * ldb, sizeof(double) * k, n_odd, s));
      else {   // row-range mode uploads the whole (small) B anyway
        MXA_HIP(copy_columns(w.d_Bstage, sizeof(double) * k, B, sizeof(double) * ldb, sizeof(double) * k, n, s));
        b_uploaded = true;
      }
    }
    if (gemm_device(h, trans, n_odd, dB + (size_t)n4 * dldb, dldb, dC + (size_t)n4 * dldc, dldc, fill_rows, s, false)) return 1;
    n = n4;
  }
  const GemmPlan p = plan_gemm(m, G.k_pad, n);
  bool tr = gemm_use_tr(p, h, trans);
  if (tr && !kmode && p.a != 8) {   // row ranges of a transposed launch are column ranges of the packed matrix: whole slabs only for the 128-row blocks of A = 8
    if (h->single) return 2;        // (a single-orientation object has no plain form for 'N': the caller's unpipelined path does this product)
    tr = false;
  }
  const PackedMatrix &GL = gemm_operand(h, trans, tr);
  int mode = gemm_default_mode(p.c);
  if (mode != 2 && mode != 3) return 2;
  { const size_t one = (size_t)p.n_pad * p.m_pad; if (partial_budget(w, one * p.splits, one) < one * p.splits) return 2; }   // partial sums beyond the budget: the grouped path of gemm_device
  if (ensure_partials(w, p, s)) return 1;
  record_geometry(h, m, k, n, p.splits, p.a, p.c, 0);
  MXA_HIP(hipMemsetAsync(w.d_denflag, 0, sizeof(int), s));   // range guard of the denormal-operand mode, raised by any K group's launch_colexp
  MXA_HIP(hipEventRecord(h->pev[0], s));
  for (hipStream_t ps : h->pipe) MXA_HIP(hipStreamWaitEvent(ps, h->pev[0], 0));   // earlier calls are done with Bp / P
  const int want_chunks = (int)std::max<size_t>(2, std::min<size_t>(kPipeChunks, std::max(b_bytes, c_bytes) >> 23));
  if (kmode) {
    const int spc = (p.splits + want_chunks - 1) / want_chunks, nch = (p.splits + spc - 1) / spc;
    for (int c = 0; c < nch; c++) {
      const int sb = c * spc, se = std::min(p.splits, sb + spc);
      const long slab0 = plan_split_begin(p, sb), slab1 = std::min<long>(p.slabs_total, plan_split_begin(p, se));
      const long k0 = std::min(k, slab0 * kSlabK), k1 = std::min(k, slab1 * kSlabK);
      if (!b_local && k1 > k0)
        MXA_HIP(copy_columns(w.d_Bstage + k0, sizeof(double) * k, B + k0, sizeof(double) * ldb, sizeof(double) * (k1 - k0), n, s));
      MXA_HIP(hipEventRecord(h->pev[2 + c], s));
      hipStream_t cs = h->pipe[c & 1];
      MXA_HIP(hipStreamWaitEvent(cs, h->pev[2 + c], 0));
      int *d_Ec = w.d_exp + (size_t)c * n;
      if (launch_colexp(dB + k0, dldb, k1 - k0, n, w.d_colpart + (size_t)c * 128 * n, d_Ec, 0, cs, w.d_denflag, kDenMaxSpan, -100000, false)) return 1;
      if (launch_pack_B(dB, dldb, k, n, w.d_Bp, G.k_pad, p.n_pad, p.c, cs, {.d_E = d_Ec, .S0 = slab0 * kSlabSteps, .S_cnt = (slab1 - slab0) * kSlabSteps, .rowscale = mode == 3 && !tr})) return 1;
      if (launch_gemm(GL, w.d_Bp, w.d_P, p, mode, cs, next_ctr(w), {.split_begin = sb, .split_end = se, .tr = tr})) return 1;
      MXA_HIP(hipEventRecord(h->pev[10 + c], cs));
    }
    for (int c = 0; c < nch; c++) MXA_HIP(hipStreamWaitEvent(s, h->pev[10 + c], 0));
    if (centered && launch_colsums(dB, dldb, k, n, trans ? nullptr : h->d_f, d_sumscratch, d_sumB, d_sumfB, s)) return 1;
    if (launch_finish(w.d_P, p, m, n, dC, dldc, fill_rows, trans ? 1 : 0, centered, d_sumB, d_sumfB, h->d_f, s, {.d_E = w.d_exp, .e_splits = spc, .e_stride = n})) return 1;
    if (!c_local) MXA_HIP(copy_columns(C, sizeof(double) * ldc, dC, sizeof(double) * fill_rows, sizeof(double) * fill_rows, n_all, s));
  } else {
    if (!b_local && !b_uploaded) MXA_HIP(copy_columns(w.d_Bstage, sizeof(double) * k, B, sizeof(double) * ldb, sizeof(double) * k, n, s));
    if (launch_colexp(dB, dldb, k, n, w.d_colpart, w.d_exp, 0, s, w.d_denflag, kDenMaxSpan, -100000, false)) return 1;
    if (launch_pack_B(dB, dldb, k, n, w.d_Bp, G.k_pad, p.n_pad, p.c, s, {.d_E = w.d_exp, .rowscale = mode == 3 && !tr})) return 1;
    if (centered && launch_colsums(dB, dldb, k, n, trans ? nullptr : h->d_f, d_sumscratch, d_sumB, d_sumfB, s)) return 1;
    MXA_HIP(hipEventRecord(h->pev[1], s));
    const long rows_chunk = ((m + want_chunks - 1) / want_chunks + kRowAlign - 1) / kRowAlign * kRowAlign;
    {   // the row ranges pad to whole row blocks each: a few blocks more than the one-launch plan
      size_t total = 0;
      for (long r0 = 0; r0 < m; r0 += rows_chunk) { const GemmPlan pc = plan_gemm(std::min(m, r0 + rows_chunk) - r0, G.k_pad, n, &p); total += (size_t)pc.splits * pc.n_pad * pc.m_pad; }
      if (total > w.cap_P) { MXA_HIP(hipStreamSynchronize(s)); if (grow(&w.d_P, &w.cap_P, total)) return 1; }
    }
    size_t p_off = 0;
    int nch = 0;
    for (long r0 = 0; r0 < m; r0 += rows_chunk, nch++) {
      const int c = nch;
      const long r1 = std::min(m, r0 + rows_chunk), rows_c = r1 - r0;
      const bool last = r1 == m;
      PackedMatrix V = GL;   // output rows [r0, r1): whole 256-row tiles, so the view starts at a tile boundary of the tiled layout
      if (!tr) {
        V.d = G.d + (size_t)(r0 / kTileRows) * G.nslabs * kTileBytes;
        V.rows = rows_c; V.rows_pad = last ? G.rows_pad - r0 : rows_chunk;
      } else V.d = GL.d + (size_t)(r0 / kSlabK) * kTileBytes;   // transposed: the output rows are the packed COLUMNS -- the view starts at slab r0 / 128 of every tile row (same pitch)
      const GemmPlan pc = plan_gemm(rows_c, G.k_pad, n, &p);   // the one-launch plan's K pieces: identical sums
      const size_t p_need = (size_t)pc.splits * pc.n_pad * pc.m_pad;
      if (p_off + p_need > w.cap_P) { set_error(4, "internal: partial-result workspace too small for the row-range pipeline"); return 1; }
      hipStream_t cs = h->pipe[c & 1];
      MXA_HIP(hipStreamWaitEvent(cs, h->pev[1], 0));
      if (launch_gemm(V, w.d_Bp, w.d_P + p_off, pc, mode, cs, next_ctr(w), {.tr = tr})) return 1;
      const long fill_c = last ? fill_rows - r0 : rows_c;
      if (launch_finish(w.d_P + p_off, pc, rows_c, n, dC + r0, dldc, fill_c, trans ? 1 : 0, centered, d_sumB, d_sumfB, (h->d_f && trans) ? h->d_f + r0 : h->d_f, cs, {.d_E = w.d_exp})) return 1;
      MXA_HIP(hipEventRecord(h->pev[10 + c], cs));
      p_off += p_need;
    }
    for (int c = 0; c < nch; c++) {
      const long r0 = (long)c * rows_chunk, r1 = std::min(m, r0 + rows_chunk);
      const long cnt = (r1 == m) ? fill_rows - r0 : r1 - r0;
      MXA_HIP(hipStreamWaitEvent(s, h->pev[10 + c], 0));
      if (!c_local) MXA_HIP(copy_columns(C + r0, sizeof(double) * ldc, dC + r0, sizeof(double) * fill_rows, sizeof(double) * cnt, n_all, s));
    }
  }
  MXA_HIP(hipStreamSynchronize(s));
  // a column outside the range of the denormal-operand mode (kDenMaxSpan; absurd inputs): the plain path redoes the product with its
  // on-device fallback
  int den = 0;
  MXA_HIP(hipMemcpy(&den, w.d_denflag, sizeof(int), hipMemcpyDeviceToHost));
  return den ? 2 : 0;
}

int refuse_while_staging(const Handle *h, const char *who) {
  if (!h->staging) return 0;
  set_error(19, "%s: the object is still being staged (%ld of %ld SNP rows appended); call mxa_plink2compressed_end first", who, h->staged_rows, h->snps);
  return 1;
}

// ---- operands that are not memory of the object's device: host memory, or memory of another GPU (peer copy over xGMI)
// *devno >= 0 and not local: the memory of another device
static bool is_local(const Handle *h, const void *p, int *devno) { return ptr_location(p, devno) == 1 && *devno == h->device; }
// The dense rows x n copy of a non-local B (ld ldb) in the staging buffer, grown to stage_elems doubles; foreign_dev >= 0: B is another device's memory and its
// producer is awaited first (sync_foreign_producer).  timed: ev_in brackets the copy (harvest_copies reads it) and the phase clock is marked.
static int upload_operand(Handle *h, const double *B, long ldb, long rows, int n, size_t stage_elems, int foreign_dev, bool timed) {
  Workspace &w = h->ws; hipStream_t s = h->stream;
  if (grow(&w.d_Bstage, &w.cap_Bstage, stage_elems)) return 1;
  clock_mark("grow-Bstage");
  if (foreign_dev >= 0 && sync_foreign_producer(foreign_dev)) return 1;
  if (timed) MXA_HIP(hipEventRecord(h->ev_in[0], s));
  MXA_HIP(copy_columns(w.d_Bstage, sizeof(double) * rows, B, sizeof(double) * ldb, sizeof(double) * rows, n, s));
  if (timed) { MXA_HIP(hipEventRecord(h->ev_in[1], s)); h->in_pending = true; }
  clock_mark("upload-B");
  return 0;
}
// its counterpart: the dense rows x n result in the staging buffer goes to a non-local C (ld ldc); timed: ev_out brackets the copy
static int download_result(Handle *h, double *C, long ldc, long rows, int n, bool timed) {
  hipStream_t s = h->stream;
  if (timed) MXA_HIP(hipEventRecord(h->ev_out[0], s));
  MXA_HIP(copy_columns(C, sizeof(double) * ldc, h->ws.d_Cstage, sizeof(double) * rows, sizeof(double) * rows, n, s));
  if (timed) { MXA_HIP(hipEventRecord(h->ev_out[1], s)); h->out_pending = true; }
  clock_mark("download-C");
  return 0;
}

int gemm_any(Handle *h, bool trans, int n, const double *B, long ldb, double *C, long ldc, long fill_rows, bool sync, bool timing) {
  if (refuse_while_staging(h, "dgemm_compressed")) return 1;
  MXA_HIP(hipSetDevice(h->device));
  const PackedMatrix &G = trans ? h->snp_major : h->ind_major;
  const long m = G.rows, k = G.k;
  if (n <= 0) return 0;
  if (!B || !C) { set_error(1, "dgemm_compressed: B and C must not be NULL"); return 1; }
  if (check_product(h, false, ldb, k, ldc, m)) return 1;
  hipStream_t s = h->stream;
  // phase clock of the call (PRINT_LEVEL > 0 / print_details): one line per call, see CallClock
  CallClock clk;
  clk.start(sync && env_print_level() > 0);   // (the environment only: the reference harness passes print_details = 1, and its timed loop should not print)
  struct ClockScope {
    CallClock *prev; CallClock &c; bool trans; int n;
    ClockScope(CallClock &c_, bool t, int n_) : prev(tl_call_clock), c(c_), trans(t), n(n_) { tl_call_clock = &c; }
    ~ClockScope() { char head[96]; snprintf(head, sizeof(head), "dgemm_compressed '%c' n=%d%s", trans ? 'T' : 'N', n, tl_in_warmup ? " (warm-up inside plink2compressed)" : ""); c.report(head); tl_call_clock = prev; }
  } clock_scope(clk, trans, n);
  int b_devno = -1, c_devno = -1;
  const bool b_local = is_local(h, B, &b_devno), c_local = is_local(h, C, &c_devno);
  clk.mark("locate");
  if (b_devno >= 0 && !b_local && sync_foreign_producer(b_devno)) return 1;   // B may still be being produced on the other device's default stream
  if (sync && (!b_local || !c_local)) {   // an operand in host memory or on another GPU, synchronous call: transfers hidden behind the product when they are large
    const int rcp = gemm_host_pipelined(h, trans, n, B, ldb, !b_local, b_local, C, ldc, !c_local, c_local, fill_rows);
    if (rcp != 2) { clk.mark("pipelined"); return rcp; }
  }
  const double *dB = B; long dldb = ldb;
  double *dC = C; long dldc = ldc;
  Workspace &w = h->ws;
  if (!b_local || !c_local) {
    harvest_copies(h);
    for (hipEvent_t *e : {&h->ev_in[0], &h->ev_in[1], &h->ev_out[0], &h->ev_out[1]}) if (!*e) MXA_HIP(hipEventCreate(e));
    clk.mark("copy-events");
  }
  if (!b_local) {   // (a foreign producer of B was awaited above, ahead of the pipelined attempt)
    if (upload_operand(h, B, ldb, k, n, (size_t)k * n, -1, true)) return 1;
    dB = w.d_Bstage; dldb = k;
  }
  if (!c_local) {
    if (grow(&w.d_Cstage, &w.cap_Cstage, (size_t)fill_rows * n)) return 1;
    dC = w.d_Cstage; dldc = fill_rows;
    clk.mark("grow-Cstage");
  }
  if (gemm_device(h, trans, n, dB, dldb, dC, dldc, fill_rows, s, timing)) return 1;
  clk.mark("enqueued");
  if (!c_local && download_result(h, C, ldc, fill_rows, n, true)) return 1;
  if (sync) {
    MXA_HIP(hipStreamSynchronize(s));
    clk.mark("stream-wait");
    harvest_profile(h);
    if (clk.on) {   // device-side durations of the same call, from the events that are there anyway
      char tmp[96];
      snprintf(tmp, sizeof(tmp), " | device: kernel %.3f in %.3f out %.3f", h->prof.launches ? h->prof_last_kernel_ms : 0.0, h->prof_last_in_ms, h->prof_last_out_ms);
      if (clk.len < (int)sizeof(clk.line) - 100) clk.len += snprintf(clk.line + clk.len, sizeof(clk.line) - clk.len, "%s", tmp);
    }
  }
  return 0;
}

// out (indiv x n) = Zc * (Zc^T * V): the 'T' then the 'N' product with the snps x n intermediate kept in HBM
int gram_any(Handle *h, int n, const double *V, long ldv, double *out, long ldo, bool sync) {
  if (refuse_while_staging(h, "mxa_gram_matvec")) return 1;
  MXA_HIP(hipSetDevice(h->device));
  const long snps = h->snps, indiv = h->indiv;
  if (n <= 0) return 0;
  if (!V || !out) { set_error(1, "mxa_gram_matvec: V and out must not be NULL"); return 1; }
  if (ldv < indiv || ldo < indiv) { set_error(7, "mxa_gram_matvec: leading dimension too small (ldv %ld, ldo %ld < %ld)", ldv, ldo, indiv); return 1; }
  hipStream_t s = h->stream;
  Workspace &w = h->ws;
  int v_devno = -1, o_devno = -1;
  const bool v_local = is_local(h, V, &v_devno), o_local = is_local(h, out, &o_devno);
  const double *dV = V; long dldv = ldv;
  double *dO = out; long dldo = ldo;
  if (!v_local) {   // (sized by max(snps, indiv), not by V: either product of the object then finds room without growing the buffer again; untimed, like both products)
    if (upload_operand(h, V, ldv, indiv, n, (size_t)std::max(snps, indiv) * n, v_devno, false)) return 1;
    dV = w.d_Bstage; dldv = indiv;
  }
  if (!o_local) {
    if (grow(&w.d_Cstage, &w.cap_Cstage, (size_t)ldo * n)) return 1;
    dO = w.d_Cstage; dldo = ldo;
  }
  if (grow(&w.d_tmp, &w.cap_tmp, (size_t)snps * n)) return 1;
  if (gemm_device(h, true, n, dV, dldv, w.d_tmp, snps, snps, s, false)) return 1;
  if (gemm_device(h, false, n, w.d_tmp, snps, dO, dldo, dldo, s, false)) return 1;
  if (!o_local && download_result(h, out, ldo, ldo, n, false)) return 1;   // (the staged result has the caller's ld: one dense copy, padding rows included)
  if (sync) MXA_HIP(hipStreamSynchronize(s));
  return 0;
}

}  // namespace mxa
