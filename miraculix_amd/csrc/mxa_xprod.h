// mxa_xprod.h -- what the crossproduct unit (mxa_crossprod.hip) shares with the units built on its tile kernels: the windowed LD entries (mxa_ldwindow.hip),
// LD pruning (mxa_ldprune.hip) and the LD operator object (mxa_ldop.hip).  Device side: the tile constants, the epilogue kinds and their argument block, the
// LD maps, the window objects with the one window store, and the layout of a count slot with its writer and its reader -- header-inline, the library is built
// without relocatable device code.  Host side: the RAII holders, the geometry and tile lists of a call, and the staging / statistics / launch helpers that
// mxa_crossprod.hip defines.
#pragma once
#include <algorithm>
#include <vector>
#include "mxa_internal.h"

namespace mxa {

// ---- tile geometry of the crossproduct kernels
constexpr int kXT = 256;              // tile edge (rows of X per operand block)
constexpr int kXStageK = 128;         // genotypes per LDS stage = 32 packed bytes per row
constexpr int kXStageBytes = kXStageK / 4;
constexpr int kXOpBytes = kXT * kXStageBytes;     // 8 KiB per operand per stage
constexpr int kXBufBytes = 2 * kXOpBytes;
// The lane <-> element map of a wave's 32 x 32 accumulator block (the MFMA's C/D layout), for every epilogue and every reader of the count slots:
// column = lane & 31, row = xacc_row(reg, rq) for accumulator register reg of the lane, rq = 4 * (lane >> 5): the two 32-lane halves hold rows 4 apart.
__device__ __forceinline__ constexpr int xacc_row(int reg, int rq) { return (reg & 3) + 8 * (reg >> 2) + rq; }

// Element-wise map applied by the epilogue (round 3: the GRM / LD post-processing of the reference's binding, crossproduct.jl:83-152, FUSED into
// the crossproduct -- SURVEY.md 8f-3 -- instead of three more passes over the 8 n^2-byte result).  Everything the map needs is known BEFORE the
// product: the column sums of M = X X^T are X (X^T 1) and its diagonal is the row-wise sum of squares, both exact integers computed from the staged
// 2-bit matrix (k_x_colsum, k_x_rowstats).  The same two functions serve the unfused kernels (k_grm_update, k_ld_center / k_ld_scale: kept for
// MXA_XPROD_FUSED_POST=0 and as the bit-identity check of the tests): i = row index, j = column index of the element as stored.
// The epilogue kinds: the POST argument of the kernels and the post_kind of their launchers (plain ints, so that the kernels' symbols stay what they were).
// kPostGrm and kPostLd are also the `post` of crossprod_any.
constexpr int kPostNone = 0;        // the plain crossproduct
constexpr int kPostGrm = 1;         // GRM map
constexpr int kPostLd = 2;          // LD map
constexpr int kPostLdBand = 3;      // windowed LD: the LD map into band storage
constexpr int kPostLdScores = 4;    // windowed LD: the LD map reduced to per-SNP scores
constexpr int kPostCounts = 5;      // pairwise-complete LD: the raw counts into a scratch slot
constexpr int kPostKinds = 6;
struct XPost {
  const double *u = nullptr;      // GRM: column sums cs of M;  LD: allele frequencies f
  const double *w = nullptr;      // LD: 1 / sigma
  const double *scal = nullptr;   // GRM: scal[0] = sum(cs), scal[1] = 2 sum f (1 - f)
  double a = 0.0;                 // GRM: 1 / n;  LD: 4 * indiv
  int do_scale = 0;
  const int *last = nullptr;      // kPostLdBand, kPostLdScores: the general window's ends last[] (LdVarWindow; nullptr: the fixed window) ...
  const long *rowptr = nullptr;   // ... and the row starts of its ragged storage; read by no other instantiation
};
// The two divisions of the reference (by the scalar c, by sigma_i and sigma_j) are multiplications by reciprocals formed once (<= 1 ulp from the
// quotient; the stated tolerance of this path is 1e-12): an fp64 division is ~15 instructions on the pipe the epilogue shares with nothing else.
// Every map is symmetric in (i, j) bit for bit -- the per-index operands are combined by a commutative operation first -- so that element (i, j) and
// element (j, i) of a GRM / LD result are equal (the reference's order, two rank-1 updates one after the other, rounds them differently).
__device__ __forceinline__ double ld_center_map(double v, double f_i, double f_j, double four_indiv) { return fma(-four_indiv, f_i * f_j, v); }   // syr!('U', -4 indiv, f, M)
__device__ __forceinline__ double ld_scale_map(double v, double is_i, double is_j) { return v * (is_i * is_j); }                                  // M ./= sigma; M ./= sigma' (is = 1 / sigma)

typedef float v16f __attribute__((ext_vector_type(16)));
// the result is written once and never read by this kernel: non-temporal stores keep the 8 n^2 bytes from displacing the packed operand tiles, which ~n/256
// tiles re-read, in the L2s and the Infinity Cache (MXA_XPROD_NT_STORE=0 at compile time: plain stores, for an A/B; round 3: docs/HISTORY.md)
#ifndef MXA_XPROD_NT_STORE
#define MXA_XPROD_NT_STORE 1
#endif
__device__ __forceinline__ void xstore(double *p, double v) {
#if MXA_XPROD_NT_STORE
  __builtin_nontemporal_store(v, p);
#else
  *p = v;
#endif
}
// ---- windowed LD (mxa_ld_band, mxa_ld_scores; by distance: mxa_ld_window_rows, mxa_ld_window_scores): the LD map of kPostLd on the tiles of a window,
// written as band storage or ragged rows (kPostLdBand), or reduced to per-SNP scores (kPostLdScores).  These two instantiations reuse the kernels' arguments:
// ans = the band / the rows / the partial buffer P, ld = its leading dimension ldb / the row stride of P, c0 = the window, post.do_scale = kind / adjust.
// The general window arrives in post.last and post.rowptr (c0 = the ndiag of P then); post.last == nullptr is the fixed window: one wave-uniform branch.
// tile diagonals dt = J - I a window touches: tile (I, J) holds the offsets j - i in [256 dt - 255, 256 dt + 255], so it meets the band iff
// 256 dt - 255 <= window, i.e. dt <= (window + 255) / 256 = ceil(window / 256) -- one more diagonal than window / 256 unless the window ends on a tile edge
__host__ __device__ __forceinline__ int ld_band_diagonals(long window) { return (int)((window + 255) / 256); }
// The window, in one place, as a small object with two instances.  in(i, j): element (i, j), i <= j < n, of R belongs to the window of i; beyond(i_base, j_base, n),
// wave-uniform: no row of the 32-row sub-block that starts at row i_base reaches column j_base >= i_base (i_base or j_base may lie in the padding at or
// beyond n: nothing is indexed out of range); at(gi, gj, ld): where row gi stores its element gj; ndiag(): tile diagonals in the scores' partial buffer.
// Fixed (mxa_ld_band, mxa_ld_scores and the pairwise pair): `window` SNPs on each side; the band band[(gj - gi) + gi * ld].
struct LdFixedWindow {
  long window;
  __device__ __forceinline__ bool in(long i, long j) const { return j - i <= window; }
  __device__ __forceinline__ bool beyond(long i_base, long j_base, long) const { return !in(i_base + 31, j_base); }
  __device__ __forceinline__ size_t at(long gi, long gj, long ld) const { return (size_t)(gj - gi) + (size_t)gi * ld; }
  __device__ __forceinline__ int ndiag() const { return ld_band_diagonals(window); }
};
// General (mxa_ld_window_*): j is in the window of i <= j iff j <= last[i], with i <= last[i] < n non-decreasing (base pairs, centimorgans, SNP counts and
// chromosome ends alike: mxa_ld_window_bounds); ragged rows rows[(gj - gi) + rowptr[gi]], rowptr = the exclusive prefix sum of last[i] - i + 1.  A sub-block
// is judged by its last row below n (last is non-decreasing); with i_base >= n that is row n - 1, whose last[n - 1] = n - 1 < i_base <= j_base.
struct LdVarWindow {
  const int *__restrict__ last;
  const long *__restrict__ rowptr;
  int nd;
  __device__ __forceinline__ bool in(long i, long j) const { return j <= (long)last[i]; }
  __device__ __forceinline__ bool beyond(long i_base, long j_base, long n) const { return j_base > (long)last[min(i_base + 31, n - 1)]; }
  __device__ __forceinline__ size_t at(long gi, long gj, long) const { return (size_t)(gj - gi) + (size_t)rowptr[gi]; }
  __device__ __forceinline__ int ndiag() const { return nd; }
};
// partial buffer of the scores: P[side][dt][row], side 0 = the tile's I rows (sums over gj), side 1 = its J rows (sums over gi; off the diagonal only)
__host__ __device__ __forceinline__ size_t ld_score_slot(int side, int dt, int ndiag, long stride) { return ((size_t)side * (size_t)(ndiag + 1) + (size_t)dt) * (size_t)stride; }
constexpr int kXScratchBytes = 4 * 32 * 33 * 8;   // the four waves' 32 x 33 epilogue scratch; the score reduction area lies behind it

// The one store of the windowed entries: the only place that knows the band layout, the window tests, the summation order and the slots of P.  It serves the
// crossproduct kernels (xprod_store_window below) and the combine kernel of the pairwise-complete entries (k_ld_pw_combine) alike: prep(a, b) readies the
// lane's sub-block (a, b); val(a, b, r) is what goes to the LDS scratch for the element that accumulator register r of that sub-block holds in the crossproduct
// kernels; fin(v, i, j) finishes a value read back from the scratch into the band entry (kPostLdBand; squared: v * v is stored) or the score term
// (kPostLdScores) of element (i, j), i, j < n.  SCORES: the reduction, else the store; win: the window object (LdFixedWindow, LdVarWindow).
// The row of register r is xacc_row(r, rq) written out: through the helper the eight windowed crossproduct kernels get another register allocation (other
// spills in prologue and epilogue), and their code is compared instruction for instruction against the build before.
template <bool SCORES, typename Win, typename Prep, typename Val, typename Fin>
__device__ __forceinline__ void ld_window_store(const Win win, Prep prep, Val val, Fin fin, bool squared, char *smem, int wave, int lane, int wi, int wj, long i0, long j0,
                                                long n, double *__restrict__ out, long ld) {
  double *scratch = reinterpret_cast<double *>(smem) + wave * (32 * 33);
  const int col = lane & 31, hh = lane >> 5, rq = 4 * hh;
  if constexpr (!SCORES) {
    // band storage band[(gj - gi) + gi * ld]: for fixed gi the band row is contiguous along gj, and the direct image runs its lanes along gj
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const long gi_base = i0 + wi * 128 + a * 32, gj_base = j0 + wj * 128 + b * 32;
        const long gj = gj_base + col;
        if (gj_base + 31 < gi_base || win.beyond(gi_base, gj_base, n)) continue;   // wave-uniform: the sub-block lies wholly below the diagonal or beyond the band
        prep(a, b);
#pragma unroll
        for (int r = 0; r < 16; r++) scratch[((r & 3) + 8 * (r >> 2) + rq) * 33 + col] = val(a, b, r);
        if (gj < n) {
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int row = (r & 3) + 8 * (r >> 2) + rq;
            const long gi = gi_base + row;
            if (gi <= gj && win.in(gi, gj)) {
              const double v = fin(scratch[row * 33 + col], gj, gi);
              xstore(&out[win.at(gi, gj, ld)], squared ? v * v : v);
            }
          }
        }
      }
  } else {
    // scores: t(r) summed along the rows of the tile (for its I rows) and, off the diagonal, along its columns (for its J rows); every sum in a fixed order:
    // a lane over its elements, then (hh 0 + hh 1) + (second wave's hh 0 + hh 1) through the LDS; one store per slot, no atomics
    const bool diag_tile = i0 == j0;
    double rowacc[4] = {0.0, 0.0, 0.0, 0.0}, colacc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const long gi_base = i0 + wi * 128 + a * 32, gj_base = j0 + wj * 128 + b * 32;
        const long gj = gj_base + col, gi = gi_base + col;
        // wave-uniform: no element of the sub-block is within the window (on the diagonal tile both triangles count: |gj - gi| <= window)
        if (gj_base >= gi_base ? win.beyond(gi_base, gj_base, n) : win.beyond(gj_base, gi_base, n)) continue;
        prep(a, b);
#pragma unroll
        for (int r = 0; r < 16; r++) scratch[((r & 3) + 8 * (r >> 2) + rq) * 33 + col] = val(a, b, r);
        if (!diag_tile && gj < n) {                            // J side: lane = column gj, its 16 rows gi (gi < gj < n)
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int row = (r & 3) + 8 * (r >> 2) + rq;
            if (win.in(gi_base + row, gj)) colacc[b] += fin(scratch[row * 33 + col], gj, gi_base + row);
          }
        }
        if (gi < n) {                                          // I side: lane = row gi, the columns gj_base + cc of its half
#pragma unroll
          for (int it = 0; it < 16; it++) {
            const int cc = 2 * it + hh;
            const long gjj = gj_base + cc;
            if (gjj < n && win.in(min(gi, gjj), max(gi, gjj))) rowacc[a] += fin(scratch[col * 33 + cc], gi, gjj);
          }
        }
      }
    double *red = reinterpret_cast<double *>(smem + kXScratchBytes);   // red[side][wave][hh][a or b][32]
#pragma unroll
    for (int q = 0; q < 4; q++) {
      red[(((0 * 4 + wave) * 2 + hh) * 4 + q) * 32 + col] = rowacc[q];
      red[(((1 * 4 + wave) * 2 + hh) * 4 + q) * 32 + col] = colacc[q];
    }
    __syncthreads();
    const int r = threadIdx.x, half = r >> 7, q = (r >> 5) & 3, c = r & 31, dt = (int)((j0 - i0) / kXT), ndiag = win.ndiag();
    auto slot = [&](int side, int w) { return red[(((side * 4 + w) * 2 + 0) * 4 + q) * 32 + c] + red[(((side * 4 + w) * 2 + 1) * 4 + q) * 32 + c]; };
    out[ld_score_slot(0, dt, ndiag, ld) + (size_t)(i0 + r)] = slot(0, half * 2 + 0) + slot(0, half * 2 + 1);          // row i0 + r: the waves (wi = half, wj = 0, 1)
    if (!diag_tile) out[ld_score_slot(1, dt, ndiag, ld) + (size_t)(j0 + r)] = slot(1, 0 * 2 + half) + slot(1, 1 * 2 + half);   // row j0 + r: the waves (wi = 0, 1, wj = half)
  }
}

// ---- the count slot of a tile: its layout is known here and nowhere else
// Count slot (kPostCounts, the entries that go through the count scratch): the raw accumulators of a tile as int32, 65 536 ints at scratch + slot * kPwSlotInts
// (slot: the fourth field of the tile entry).  Lane-linear and register-major in quads: registers 4 q .. 4 q + 3 of sub-block (a, b) of thread t are the
// int4 at xcount_quads(scratch, slot)[xcount_quad(a, b, q)], so one 16-byte access per lane and quad, a wave moves 1 KiB contiguous; no LDS transpose.
constexpr size_t kPwSlotInts = (size_t)kXT * kXT;
__device__ __forceinline__ const int4 *xcount_quads(const int *__restrict__ scratch, int slot) { return reinterpret_cast<const int4 *>(scratch + (size_t)slot * kPwSlotInts) + threadIdx.x; }
__device__ __forceinline__ constexpr int xcount_quad(int a, int b, int q) { return ((a * 4 + b) * 4 + q) * 256; }
// the writer, from the crossproduct kernels' accumulators (FP4 engine: acc x 4, exact)
template <typename AccT>
__device__ __forceinline__ void xprod_store_counts(const AccT (&acc)[4][4], int *__restrict__ scratch, int slot) {
  int4 *p = const_cast<int4 *>(xcount_quads(scratch, slot));
  auto cnt = [](auto v) -> int { if constexpr (__is_same(AccT, v16f)) return (int)(v * 4.0f); else return v; };
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++)
#pragma unroll
      for (int q = 0; q < 4; q++)
        p[xcount_quad(a, b, q)] = make_int4(cnt(acc[a][b][4 * q]), cnt(acc[a][b][4 * q + 1]), cnt(acc[a][b][4 * q + 2]), cnt(acc[a][b][4 * q + 3]));
}
// the reader: counts[k][reg] = what accumulator register reg of this lane held in sub-block (a, b) of the tile in slot + k, for the SLOTS products of a window tile
template <int SLOTS>
__device__ __forceinline__ void ld_load_counts(const int *__restrict__ scratch, int slot, int a, int b, int (&counts)[SLOTS][16]) {
  const int4 *p = xcount_quads(scratch, slot);
#pragma unroll
  for (int q = 0; q < 4; q++)
#pragma unroll
    for (int k = 0; k < SLOTS; k++) {
      const int4 w = p[(size_t)k * (kPwSlotInts / 4) + xcount_quad(a, b, q)];
      counts[k][4 * q] = w.x; counts[k][4 * q + 1] = w.y; counts[k][4 * q + 2] = w.z; counts[k][4 * q + 3] = w.w;
    }
}

// ---- host side
struct XEvent {   // RAII: events, streams and device buffers are released on every exit path
  hipEvent_t e = nullptr;
  ~XEvent() { if (e) (void)hipEventDestroy(e); }
  int create(unsigned flags = hipEventDefault) { MXA_HIP(hipEventCreateWithFlags(&e, flags)); return 0; }
};
struct XStream {
  hipStream_t s = nullptr;
  ~XStream() { if (s) (void)hipStreamDestroy(s); }
  int create(unsigned flags) { MXA_HIP(hipStreamCreateWithFlags(&s, flags)); return 0; }
};
struct XBuf {
  void *p = nullptr;
  ~XBuf() { if (p) (void)hipFree(p); }
  int alloc(size_t bytes) { MXA_HIP(hipMalloc(&p, bytes ? bytes : 1)); return 0; }
  void release() { if (p) { (void)hipFree(p); p = nullptr; } }
};
// Geometry of one call: X has `rows` rows, staged as nb tiles of 256 rows; a staged row is nslabs slabs of 128 genotypes (32 bytes, the pitch), one
// K stage of the kernels each.
struct XGeom {
  long rows;
  int nb, stages;
  long nslabs;
  XGeom(long k, long r) : rows(r), nb((int)((r + kXT - 1) / kXT)), stages((int)((k + kXStageK - 1) / kXStageK)), nslabs(stages) {}
  long rows_pad() const { return (long)nb * kXT; }
  size_t pitch() const { return (size_t)nslabs * kXStageBytes; }
};

// The tile lists of a call's chunks, uploaded once: chunk c is d_tiles[first[c], first[c + 1]), in the gang order where gang_order_tiles took it (xcd[c]).
// d_gang: the gangs' 32 control counters, then mid_cap ints for the counters of their meetings inside a tile, sized for the longest list.
struct XTiles {
  std::vector<int4> tiles;
  std::vector<size_t> first;
  std::vector<char> xcd;
  size_t mid_cap = 0;
  XBuf d_tiles, d_gang;
  int launch(int c, const XGeom &g, bool f4, hipStream_t s, const uint8_t *d_X, double *d_ans, long ld, long c0, unsigned long long *d_diag, int post_kind,
             const XPost &post) const;   // mxa_crossprod.hip: the kernels live there
};

// mxa_crossprod.hip (the comments are at the definitions)
int upload_tiles(std::vector<std::vector<int4>> chunks, hipStream_t s, XTiles &t);
std::vector<int4> window_tiles(const std::vector<int> &jmax);
int stage_operand(const unsigned char *snp_matrix, bool in_dev, long row_bytes, bool is_plink, const XGeom &g, uint8_t *d_X, int *d_has3, XBuf &bounce,
                  hipStream_t s, long planes_indiv = 0, long mask_fields = 0);
int pick_engine(const int *d_has3, long k, hipStream_t s, bool &f4);
int fused_post_stats(const XGeom &g, const uint8_t *d_X, long k, int post, int do_scale, const double *d_f, XBuf (&st)[3], hipStream_t s, XPost &xp);
dim3 rowstats_grid(const XGeom &g, long *spc);
hipError_t profile_launch(const XEvent &e0, const XEvent &e1);
constexpr long kXFusedMaxRows = 29000000L;   // k_x_rowstats: 16 * 3 * (3 rows) must fit 32 bits
constexpr long kPwMaxIndiv = 47453132L;      // the pairwise-complete entries: 4 indiv^2 < 2^53

// mxa_ldwindow.hip: both routes of the CSR entries, also run twice by the window pruning entries (mxa_ldprune.hip) on device arrays of the library's own
int ld_pairs_any(const char *who, const unsigned char *plink, long snps, long indiv, const int *last, double min_r2, int kind, long *rowptr, int *col, double *val,
                 long capacity, long *total, bool pairwise, bool is_plink, const double *freq, bool no_val = false);
}  // namespace mxa
