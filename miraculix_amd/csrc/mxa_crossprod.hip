// mxa_crossprod.hip -- integer crossproduct M = X * X^T on the matrix cores, exact.
//
// Replaces src/cuda/snp_multiply_cuda.cu:38-382 of the reference (CUTLASS u4 TensorOp GEMM with the two-MMA 2-bit trick
// snp_multiply_cuda.h:121-199, per-tile PCIe re-uploads, host int32->double mirror loop) with a device-resident design:
// X is staged once (2 bits per value, the 256-row x 32-byte tiled layout of mxa_internal.h), every upper-triangular 256x256 tile
// is one workgroup, the packed rows go HBM -> LDS by lane-linear LDS-DMA, each wave unpacks its 2-bit words in registers and the
// epilogue converts to fp64 and writes the tile and its mirror image.  Two exact engines:
//   k_crossprod_f4  (default)  v_mfma_scale_f32_32x32x64_f8f6f4 with FP4 (e2m1) operands: a 2-bit value z in {0..3} in the low bits
//                   of a nibble IS the e2m1 number z/2, so the unpack is 3 VALU per 16 values (two masks and a shift) and the
//                   instruction runs at twice the int8 rate (tools/mfma_f4_probe.hip: exact, 32.8 cycles, 8.3 Pop/s bare loop).
//                   Products are multiples of 1/4; the fp32 accumulator is exact while sum z z' < 2^24, i.e. for K < 1 864 135 with
//                   values up to 3 and K < 4 194 304 when the staged matrix holds no 3 (checked while staging).
//   k_crossprod_i8  (longer K)  v_mfma_i32_32x32x32_i8, 7 VALU per 16 values, exact int32 for K < 2.3e8; the same K-step pipeline.
#include "../../include/miraculix_amd.h"
#include "mxa_internal.h"
#include "mxa_queue.h"
#include "mxa_hostmem.h"
#include <atomic>
#include <chrono>
#include <thread>
#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

namespace mxa {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

using gptr_t = const __attribute__((address_space(1))) void *;
using lptr_t = __attribute__((address_space(3))) void *;

// ---- the reference's PLINK -> 2-bit byte table (snp_multiply_cuda.h:202-210): 00->0, 10->1, 11->2, and a byte that
// holds a missing pair (01) anywhere becomes 0xFF.  SWAR on 4 bytes at a time.
__device__ __forceinline__ uint32_t plink_lut4(uint32_t w) {
  const uint32_t H = (w >> 1) & 0x55555555u, L = w & 0x55555555u;
  const uint32_t z = ((H & L) << 1) | (H & ~L);
  uint32_t miss = L & ~H;                  // bit 2q of a byte set <=> field q is 01
  miss |= miss >> 4;                       // fold fields (0,2) and (1,3); garbage from the next byte lands in bits 4..7
  miss &= 0x05050505u;
  miss |= miss >> 2;
  miss &= 0x01010101u;                     // bit 0 of each byte: the byte holds a missing pair
  return z | (miss * 0xFFu);
}

__global__ void __launch_bounds__(256) k_plink_lut(uint32_t *__restrict__ d, size_t ndwords) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ndwords; i += (size_t)gridDim.x * blockDim.x) d[i] = plink_lut4(d[i]);
}

// copy rows (src pitch arbitrary) into the tiled layout (mxa_internal.h: byte b of row r -> ((r/256)*nslabs + b/32)*8192 + (r%256)*32
// + b%32), optionally applying the table; padding bytes/rows stay zero (the buffer is memset first).  *has3 |= 1 when a staged field
// holds the value 3 (raw 2-bit input, or a byte with a missing pair under the reference's table).
// the staging kernels' two steps.  The dword at byte b of a packed row, p = its address: one aligned non-temporal load (read once), or byte by byte at an
// unaligned address and in the row's tail; keep = the mask of the bytes that exist.
__device__ __forceinline__ uint32_t xstage_load(const uint8_t *p, long b, long row_bytes, uint32_t &keep) {
  uint32_t w = 0;
  keep = 0;
  if (b + 4 <= row_bytes && (reinterpret_cast<size_t>(p) & 3) == 0) { w = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(p)); keep = 0xFFFFFFFFu; }
  else
    for (int u = 0; u < 4; u++)
      if (b + u < row_bytes) { w |= (uint32_t)p[u] << (8 * u); keep |= 0xFFu << (8 * u); }
  return w;
}
// ... and where the dword at byte b of row R goes in the tiled layout
__device__ __forceinline__ uint32_t *xstage_dst(uint8_t *dst, long nslabs, long R, long b) {
  return reinterpret_cast<uint32_t *>(dst + ((size_t)(R / kTileRows) * nslabs + (size_t)(b / kSlabBytes)) * kTileBytes + (size_t)(R % kTileRows) * kSlabBytes + b % kSlabBytes);
}
// fields > 0 (the GRM / LD entries): the row holds `fields` 2-bit fields; those at and beyond it -- the padding bits of the row's last byte -- are set to 00
// BEFORE the table, so that a padding 01 cannot turn its byte into 0xFF.  fields == 0 (the plain crossproduct): the bytes as stored, as the reference multiplies them.
__global__ void __launch_bounds__(256) k_xstage(const uint8_t *__restrict__ src, size_t src_pitch, long row_bytes, long nrows,
                                                uint8_t *__restrict__ dst, long nslabs, long dst_row0, int apply_lut, int *__restrict__ has3, long fields) {
  const long dpr = (row_bytes + 3) / 4;
  const long total = nrows * dpr;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const long r = idx / dpr, d = idx - r * dpr, b = d * 4;
    uint32_t keep, w = xstage_load(src + (size_t)r * src_pitch + b, b, row_bytes, keep);
    if (fields > 0) {
      const long left = fields - 4 * b;                                         // fields from this dword's first one on
      if (left < 16) w &= left > 0 ? (1u << (2 * left)) - 1u : 0u;
    }
    if (apply_lut) w = plink_lut4(w) & keep;
    if (w & (w >> 1) & 0x55555555u) atomicOr(has3, 1);
    *xstage_dst(dst, nslabs, dst_row0 + r, b) = w;
  }
}

// Pairwise-complete LD (mxa_ld_band_pairwise, mxa_ld_scores_pairwise): the PLINK codes of a row as THREE planes in the tiled layout, stacked as one operand
// of 3 * rows_pad rows (plane p starts plane_bytes * p behind dst, so tile index p * nb + I addresses block I of plane p):
//   plane 0  Z: 00 -> 0, 01 -> 0, 10 -> 1, 11 -> 2   (allele count, missing as 0)
//   plane 1  M: 01 -> 0, else 1                        (genotype present)
//   plane 2  A: 11 -> 1, else 0                        (z^2 = z + 2 a)
// Fields at and beyond `indiv` -- the padding bits of a row's last byte, which read as 00 in a well-formed file -- are no individuals: they get 0 in every
// plane, M included (else every N_ij would count them).  *has_missing |= 1 when a 01 occurs among the individuals: one atomic per wave, not per dword.
__global__ void __launch_bounds__(256) k_xstage_planes(const uint8_t *__restrict__ src, size_t src_pitch, long row_bytes, long nrows, long indiv,
                                                       uint8_t *__restrict__ dst, long nslabs, size_t plane_bytes, long dst_row0, int *__restrict__ has_missing) {
  const long dpr = (row_bytes + 3) / 4;
  const long total = nrows * dpr;
  uint32_t seen = 0;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const long r = idx / dpr, d = idx - r * dpr, b = d * 4;
    uint32_t keep;
    const uint32_t w = xstage_load(src + (size_t)r * src_pitch + b, b, row_bytes, keep);
    const long left = indiv - 4 * b;                                            // individuals from this dword's first field on (> 0: b < row_bytes)
    const uint32_t vm = left >= 16 ? 0x55555555u : ((1u << (2 * left)) - 1u) & 0x55555555u;
    const uint32_t H = (w >> 1) & vm, L = w & vm, miss = L & ~H;
    seen |= miss;
    uint32_t *q = xstage_dst(dst, nslabs, dst_row0 + r, b);
    q[0] = ((H & L) << 1) | (H & ~L);
    q[plane_bytes / 4] = vm & ~miss;
    q[plane_bytes / 2] = H & L;
  }
  if (__any(seen != 0) && (threadIdx.x & 63) == 0) atomicOr(has_missing, 1);
}

// ---- main kernel -----------------------------------------------------------------------------------------------
constexpr int kXT = 256;              // tile edge (rows of X per operand block)
constexpr int kXStageK = 128;         // genotypes per LDS stage = 32 packed bytes per row
constexpr int kXStageBytes = kXStageK / 4;
constexpr int kXOpBytes = kXT * kXStageBytes;     // 8 KiB per operand per stage
constexpr int kXBufBytes = 2 * kXOpBytes;

// 16 two-bit fields of a dword -> 16 int8 in 4 dwords (field order permuted identically for both operands)
__device__ __forceinline__ v4i unpack16(uint32_t w) {
  v4i r;
  r[0] = (int)(w & 0x03030303u);
  r[1] = (int)((w >> 2) & 0x03030303u);
  r[2] = (int)((w >> 4) & 0x03030303u);
  r[3] = (int)((w >> 6) & 0x03030303u);
  return r;
}

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
__device__ __forceinline__ double grm_map(double v, double cs_i, double cs_j, double inv_n, double tot_nn, double inv_c, int do_scale) {
  v = fma(-(cs_i + cs_j), inv_n, v);   // BLAS.ger!(-1/indiv, col_sum, one_vector, M); BLAS.ger!(-1/indiv, one_vector, col_sum, M)  (cs_i + cs_j: exact integers)
  v = v + tot_nn;                      // M .+= sum(col_sum) / indiv^2
  if (do_scale) v *= inv_c;            // M ./= 2 sum f (1 - f)
  return v;
}
__device__ __forceinline__ double ld_center_map(double v, double f_i, double f_j, double four_indiv) { return fma(-four_indiv, f_i * f_j, v); }   // syr!('U', -4 indiv, f, M)
__device__ __forceinline__ double ld_scale_map(double v, double is_i, double is_j) { return v * (is_i * is_j); }                                  // M ./= sigma; M ./= sigma' (is = 1 / sigma)

// Epilogue shared by both engines.  32x32 C/D map: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5); element (gi, gj) = M[gi][gj].
// The output holds columns [c0, ..) of M with leading dimension ld (whole matrix: c0 = 0, ld = n).
// Direct image: M[gj, gi] at ans[gj + (gi-c0)*ld], lanes run along gj (256-byte segments).  Mirror image M[gi, gj] at
// ans[gi + (gj-c0)*ld]: the tile is transposed through a per-wave LDS scratch (row stride 33 doubles: conflict-free both ways)
// so its lanes run along gi as well.  AccT = v16i: exact int32 sums; v16f: sums of z z' / 4 (FP4 engine), exact, times 4.
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

// The crossproduct kernels' side of it: the scratch takes the accumulators as fp64, and a value read back is mapped with the LD map of kPostLd (post.u is the
// caller's freq, of length n: fin is only ever called with i, j < n) -- into the band entry r, or the score term t(r).
template <typename AccT, int POST>
__device__ __forceinline__ void xprod_store_window(const AccT (&acc)[4][4], char *smem, int wave, int lane, int wi, int wj, long i0, long j0, long n,
                                                   double *__restrict__ out, long ld, long window, const XPost &post) {
  constexpr double scale = __is_same(AccT, v16f) ? 4.0 : 1.0;
  const bool flag = post.do_scale != 0;                                    // kind (band) / adjust (scores)
  // post.a = 4 indiv: 1 / (indiv - 2).  Formed here and not inside fin: there the gang kernels spill 648 / 764 bytes per lane (FP4 / int8) instead of 432 / 492
  constexpr bool kScores = POST == kPostLdScores;
  const double inv_adj = kScores && flag ? 1.0 / (post.a * 0.25 - 2.0) : 0.0;
  auto fin = [&](double v, long i, long j) -> double {
    const double r = ld_scale_map(ld_center_map(v, post.u[i], post.u[j], post.a), post.w[i], post.w[j]);
    if constexpr (!kScores) return r;
    else {                                                                 // every operation rounded on its own (no contraction): the tests restate this line
      const double r2 = __dmul_rn(r, r);
      return flag ? __dsub_rn(r2, __dmul_rn(__dsub_rn(1.0, r2), inv_adj)) : r2;
    }
  };
  auto store = [&](auto win) {
    ld_window_store<kScores>(win, [](int, int) {}, [&](int a, int b, int r) -> double { return (double)acc[a][b][r] * scale; }, fin, !kScores && flag, smem, wave, lane,
                             wi, wj, i0, j0, n, out, ld);
  };
  // Both instances of the store side by side behind one wave-uniform test of a kernel argument (post.last == nullptr: the fixed window); for the general one
  // `window` carries the partial buffer's ndiag.  (Choosing per sub-block instead, around the loops over the LDS scratch, puts scratch accesses into the stage loop.)
  if (post.last) store(LdVarWindow{post.last, post.rowptr, (int)window});
  else store(LdFixedWindow{window});
}

// Count store (kPostCounts, pairwise-complete LD): the raw accumulators of the tile as int32 (FP4 engine: acc x 4, exact) into the scratch slot the tile entry
// names (its fourth field), 65 536 ints.  Lane-linear and register-major in quads: registers 4 q .. 4 q + 3 of thread t at slot + q * 1024 + 4 t, one 16-byte
// store per lane and quad (a wave writes 1 KiB contiguous); no LDS transpose.  The combine kernel reads the same addresses with the same lane <-> element map.
constexpr size_t kPwSlotInts = (size_t)kXT * kXT;
template <typename AccT>
__device__ __forceinline__ void xprod_store_counts(const AccT (&acc)[4][4], int *__restrict__ scratch, int slot) {
  int4 *p = reinterpret_cast<int4 *>(scratch + (size_t)slot * kPwSlotInts) + threadIdx.x;
  auto cnt = [](auto v) -> int { if constexpr (__is_same(AccT, v16f)) return (int)(v * 4.0f); else return v; };
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++)
#pragma unroll
      for (int q = 0; q < 4; q++)
        p[((a * 4 + b) * 4 + q) * 256] = make_int4(cnt(acc[a][b][4 * q]), cnt(acc[a][b][4 * q + 1]), cnt(acc[a][b][4 * q + 2]), cnt(acc[a][b][4 * q + 3]));
}

// POST: kPostNone, kPostGrm, kPostLd (XPost above); each stored element is mapped with ITS OWN (row, column), so both images equal what
// the unfused element-wise kernels produce.  With a map the 32 x 32 block goes to the LDS scratch first (static accumulator indices) and both images
// are written by loops over IT, never over the accumulators: when the maps still held fp64 divisions, their 512-fold unrolled code exceeded the
// compiler's full-unroll budget, the loops stayed rolled, and a rolled loop over the accumulators indexes them dynamically, i.e. moves them to
// scratch memory for the whole kernel (measured: 10x).  With the reciprocal maps everything unrolls; this form stays safe if it ever does not.
template <typename AccT, int POST>
__device__ __forceinline__ void xprod_store(const AccT (&acc)[4][4], char *smem, int wave, int lane, int wi, int wj, long i0, long j0, int images, long n,
                                            double *__restrict__ ans, long ld, long c0, const XPost &post) {
  double *scratch = reinterpret_cast<double *>(smem) + wave * (32 * 33);   // the DMA ring is dead after the last barrier
  const int col = lane & 31, hh = lane >> 5, rq = 4 * hh;
  constexpr double scale = __is_same(AccT, v16f) ? 4.0 : 1.0;
  if constexpr (POST == kPostLdBand || POST == kPostLdScores) {   // windowed LD: band or row storage / scores (ans, ld, c0 = band or partial buffer, its stride, the window)
    xprod_store_window<AccT, POST>(acc, smem, wave, lane, wi, wj, i0, j0, n, ans, ld, c0, post);
  } else if constexpr (POST == kPostNone) {
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const long gi_base = i0 + wi * 128 + a * 32, gj_base = j0 + wj * 128 + b * 32;
        const long gj = gj_base + col;
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int row = (r & 3) + 8 * (r >> 2) + rq;
          const double v = (double)acc[a][b][r] * scale;
          if ((images & 1) && gi_base + row < n && gj < n) xstore(&ans[(size_t)gj + (size_t)(gi_base + row - c0) * ld], v);
          scratch[row * 33 + col] = v;
        }
        if (images & 2) {
#pragma unroll
          for (int it = 0; it < 16; it++) {
            const int cc = 2 * it + hh;                       // column of the tile = gj offset; lanes (lane&31) run along gi
            const double v = scratch[col * 33 + cc];
            const long gi = gi_base + col, gjj = gj_base + cc;
            if (gi < n && gjj < n) xstore(&ans[(size_t)gi + (size_t)(gjj - c0) * ld], v);
          }
        }
      }
  } else {
    double tot_nn = 0.0, cc_scale = 1.0;
    if (POST == kPostGrm) { tot_nn = post.scal[0] / ((double)n * (double)n); cc_scale = post.do_scale ? 1.0 / post.scal[1] : 1.0; }
    auto map = [&](double v, long i, long j) -> double {       // element M[i][j] (i, j < n)
      if (POST == kPostGrm) return grm_map(v, post.u[i], post.u[j], post.a, tot_nn, cc_scale, post.do_scale);
      return ld_scale_map(ld_center_map(v, post.u[i], post.u[j], post.a), post.w[i], post.w[j]);
    };
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const long gi_base = i0 + wi * 128 + a * 32, gj_base = j0 + wj * 128 + b * 32;
        const long gj = gj_base + col, gi = gi_base + col;
#pragma unroll
        for (int r = 0; r < 16; r++) scratch[((r & 3) + 8 * (r >> 2) + rq) * 33 + col] = (double)acc[a][b][r] * scale;
        if ((images & 1) && gj < n) {                          // direct image: row index gj, column index gi_base + row
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int row = (r & 3) + 8 * (r >> 2) + rq;
            if (gi_base + row < n) xstore(&ans[(size_t)gj + (size_t)(gi_base + row - c0) * ld], map(scratch[row * 33 + col], gj, gi_base + row));
          }
        }
        if ((images & 2) && gi < n) {                          // mirror image: row index gi, column index gj_base + cc
#pragma unroll
          for (int it = 0; it < 16; it++) {
            const int cc = 2 * it + hh;
            if (gj_base + cc < n) xstore(&ans[(size_t)gi + (size_t)(gj_base + cc - c0) * ld], map(scratch[col * 33 + cc], gi, gj_base + cc));
          }
        }
      }
  }
}

// Both engines: 4 waves, one per SIMD, wave tile 128 x 128 (16 accumulator tiles = 256 registers), one workgroup per CU.  (History: 8 waves with
// 128 x 64 wave tiles stalled at 43-54 % of the int8 peak on their unpack VALU density; the round-1/2 int8 kernel k_crossprod2 -- 3-deep ring, the
// packed words of a whole stage prefetched mid-stage -- ran 2704 cycles per stage of 2048 ideal at 2.38 GHz, issue-bound; round 3 moved the int8
// engine onto the FP4 kernel's K-step pipeline below: 2272 cycles at 2.19 GHz, now power-bound like the FP4 engine.)
__device__ __forceinline__ void xdma16_s(const void *sbase, uint32_t voff, uint32_t lds_addr) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %0" ::"s"(sbase), "v"(voff), "s"(lds_addr) : "memory", "m0");
}

// ---- FP4 engine ----------------------------------------------------------------------------------------------------------------
// Per stage of 128 genotypes TWO K-steps of 64 (v_mfma_scale_f32_32x32x64_f8f6f4, FP4
// operands, unit scales).  Lane (row r = lane&31, K half h = lane>>5) reads 16 bytes = 64 genotypes of its row per stage; K-step ks uses
// dwords 2ks, 2ks+1 of them.  A dword of 16 two-bit values z becomes two dwords of 8 nibbles 00zz -- the e2m1 numbers z/2 -- by
// (w & 0x33333333) and ((w >> 2) & 0x33333333): 6 VALU per fragment of 32 values, 48 per K-step of 16 MFMAs (the int8 engine: 56 VALU per
// 16 MFMAs of HALF the K).  The K order inside a fragment is permuted identically for both operands, so the dot product is unchanged.
typedef int v8i __attribute__((ext_vector_type(8)));
constexpr int kF4Bufs = 8;                        // ring depth of the FP4 kernel
constexpr int kF4Lds = kF4Bufs * kXBufBytes;      // 128 KiB (one workgroup per CU: 256 accumulator registers per lane)
__device__ __forceinline__ v4i unpack_f4(uint32_t w0, uint32_t w1) {
  v4i r;
  r[0] = (int)(w0 & 0x33333333u);
  r[1] = (int)((w0 >> 2) & 0x33333333u);
  r[2] = (int)(w1 & 0x33333333u);
  r[3] = (int)((w1 >> 2) & 0x33333333u);
  return r;
}
__device__ __forceinline__ v16f mfma_f4(const v4i &a, const v4i &b, const v16f &c) {
  const v8i a8 = {a[0], a[1], a[2], a[3], 0, 0, 0, 0}, b8 = {b[0], b[1], b[2], b[3], 0, 0, 0, 0};   // FP4 operands occupy 4 of the 8 registers
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, 4, 4, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);   // cbsz = blgp = 4: e2m1; scales 2^0
}

// EXP (diagnostic instantiations only, results are wrong): 1 = no unpack VALU; 2 = no DMA / barrier / LDS reads inside the loop;
// 3 = barrier only; 4 = DMA + LDS reads without the barrier; 5 = barrier + DMA, no LDS reads; 6 = barrier + LDS reads, no DMA
// The same pipeline serves the int8 engine (I8, round 3): a "K-step of 64" is then two v_mfma_i32_32x32x32_i8 sub-steps -- the lane's two dwords of
// a K-step unpack into two int8 fragments (14 VALU per sub-block instead of 6), 8 MFMAs per sub-block row instead of 4, exact int32 sums.  It replaced
// k_crossprod2 (3-deep ring, words of a whole stage prefetched mid-stage: 2704 cycles per stage of 2048 ideal at 2.38 GHz -- issue-bound, not
// power-bound).
struct FragI8 { v4i lo, hi; };
template <bool I8> struct XFrag { using type = v4i; using acc = v16f; };
template <> struct XFrag<true> { using type = FragI8; using acc = v16i; };

// second meeting point of a gang (round 4; MXA_XPROD_GANG_MID = parts of the K range: 1 = no meeting, 2 = one meeting half way, the default): the tiles of a
// gang start together but drift apart inside a 2.6 ms tile; half way through the K range every member adds to the gang's counter and waits for the others --
// bounded by the join time and by 4 % of the tile's own duration, whichever is shorter -- so that the second half streams in step again
struct GangMid { int *ctr; int target; unsigned ticks; int parts; int stride; };   // parts - 1 meetings inside a tile, meeting q uses ctr[(q - 1) * stride]
template <bool DIAG, int EXP, bool I8, int POST>
__device__ __forceinline__ void xprod_tile(const uint8_t *__restrict__ X, long nslabs, int stages, const int4 t, size_t tile_index, long n, double *__restrict__ ans,
                                           long ld, long c0, unsigned long long *__restrict__ diag, const XPost &post, const GangMid gm = GangMid{nullptr, 0, 0, 1, 0}) {
  using FragT = typename XFrag<I8>::type;
  using AccT = typename XFrag<I8>::acc;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wi = wave >> 1, wj = wave & 1;
  const long i0 = (long)t.x * kXT, j0 = (long)t.y * kXT;
  const uint32_t lds0 = (uint32_t)(size_t)(lptr_t)smem;
  const uint32_t v_lane = (uint32_t)lane * 16;
  const char *XI = reinterpret_cast<const char *>(X) + (size_t)t.x * nslabs * kTileBytes;
  const char *XJ = reinterpret_cast<const char *>(X) + (size_t)t.y * nslabs * kTileBytes;
  auto issue = [&](int stage, int buf) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int u = wave + 4 * i;
      const int op = u >> 3, uu = u & 7;
      xdma16_s((op ? XJ : XI) + (size_t)stage * kTileBytes + uu * 1024, v_lane, lds0 + buf * kXBufBytes + op * kXOpBytes + uu * 1024);
    }
  };

  AccT acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[a][b][r] = 0;

  const int a_off = (wi * 128 + (lane & 31)) * kXStageBytes + (lane >> 5) * 16;
  const int b_off = kXOpBytes + (wj * 128 + (lane & 31)) * kXStageBytes + (lane >> 5) * 16;

  // Ring of NB buffers (a stage lasts only ~0.5 us at the FP4 rate).  Stages 0 .. NB-1 are in flight at the start; at the start of stage s
  // the words of stage s are already in registers, so its buffer takes stage s + NB, and stage s + 1 is waited for (stages s+2 .. s+NB-1 stay
  // in flight).
  constexpr int NB = kF4Bufs;
#pragma unroll
  for (int i = 0; i < NB; i++) issue(min(i, stages - 1), i);   // always NB stages in flight (clamped: short K re-loads the last stage)
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (NB - 1)) : "memory");
  __syncthreads();
  unsigned long long t0 = 0, r0 = 0;
  if (DIAG) { t0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }
  // Software pipeline in K-steps t = 2 s + ks (a stage has two K-steps of 64 genotypes):
  //   during K-step t the wave (1) issues the ds_read_b64 of the packed words of K-step t+2 into word set W[t%2], (2) unpacks the words of
  //   K-step t+1 (read during t-1, word set W[(t+1)%2]) into fragment set F[(t+1)%2], 3 VALU after every MFMA, and (3) issues the 16 MFMAs
  //   of K-step t from fragment set F[t%2].  Neither an LDS latency nor a VALU result is ever waited for, and no register set is copied
  //   (the period of the alternation, two K-steps, is exactly one stage, so the stage loop needs no unrolling).
  //   Stage start: the words of stage s were all read during stage s-1, so after the barrier buffer s%NB takes stage s+NB; stage s+1
  //   must have landed (its words are read during this stage); stages s+2 .. s+NB-1 stay in flight.
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  u32x2 wa0[4], wb0[4], wa1[4], wb1[4];      // W[0] / W[1]: words of an even / odd K-step, 4 A and 4 B sub-blocks of 32 rows
  FragT fa0[4], fb0[4], fa1[4], fb1[4];      // F[0] / F[1]
  auto unpack = [](const u32x2 &w) -> FragT {
    if constexpr (I8) { FragI8 r; r.lo = unpack16(w.x); r.hi = unpack16(w.y); return r; }
    else {
      if (EXP == 1) { v4i r = {(int)w.x, (int)w.y, (int)w.x, (int)w.y}; return r; }
      return unpack_f4(w.x, w.y);
    }
  };
  auto mma = [](const FragT &fa, const FragT &fb, const AccT &c) -> AccT {
    if constexpr (I8) return __builtin_amdgcn_mfma_i32_32x32x32_i8(fa.hi, fb.hi, __builtin_amdgcn_mfma_i32_32x32x32_i8(fa.lo, fb.lo, c, 0, 0, 0), 0, 0, 0);
    else return mfma_f4(fa, fb, c);
  };
#pragma unroll
  for (int a = 0; a < 4; a++) {
    wa0[a] = *reinterpret_cast<const u32x2 *>(smem + a_off + a * 32 * kXStageBytes);
    wb0[a] = *reinterpret_cast<const u32x2 *>(smem + b_off + a * 32 * kXStageBytes);
    wa1[a] = *reinterpret_cast<const u32x2 *>(smem + a_off + a * 32 * kXStageBytes + 8);
    wb1[a] = *reinterpret_cast<const u32x2 *>(smem + b_off + a * 32 * kXStageBytes + 8);
  }
#pragma unroll
  for (int a = 0; a < 4; a++) { fa0[a] = unpack(wa0[a]); fb0[a] = unpack(wb0[a]); fa1[a] = fa0[a]; fb1[a] = fb0[a]; }
  int buf = 0;
  // K-step: MFMAs from (FA, FB); unpack (WAU, WBU) -> (FAN, FBN); read the words at LDS address RD (+ sub-block) into (WAR, WBR).
  // Everything that is not an MFMA is spread over the four groups of 4 MFMAs (one DMA unit when DO_DMA, two ds_read_b64, 12 unpack VALU per
  // group) and the whole stage is ONE basic block (no branches: the DMA of the last NB stages re-loads the final stage into buffers nobody
  // reads, the reads after the last stage hit a valid buffer), so that the instruction scheduler keeps the interleave it is given:
  // clustered at the stage start the 4 DMA issues and 16 LDS reads cost ~165 + ~140 cycles of a 1024-cycle stage (profiles/r02_mfma_f4_probe.txt).
#define MXA_F4_KSTEP(FA, FB, WAU, WBU, FAN, FBN, WAR, WBR, RD, DO_DMA)                                                                      \
  {                                                                                                                                        \
    _Pragma("unroll") for (int a = 0; a < 4; a++) {                                                                                        \
      if (DO_DMA && EXP != 2 && EXP != 3 && EXP != 6) {                                                                                    \
        const int u = wave + 4 * a, op = u >> 3, uu = u & 7;                                                                               \
        xdma16_s((op ? XJ : XI) + (size_t)dma_stage * kTileBytes + uu * 1024, v_lane, lds0 + dma_buf * kXBufBytes + op * kXOpBytes + uu * 1024); \
      }                                                                                                                                    \
      if (EXP != 2 && EXP != 3 && EXP != 5) {                                                                                              \
        WAR[a] = *reinterpret_cast<const u32x2 *>((RD) + a_off + a * 32 * kXStageBytes);                                                   \
        WBR[a] = *reinterpret_cast<const u32x2 *>((RD) + b_off + a * 32 * kXStageBytes);                                                   \
      }                                                                                                                                    \
      FAN[a] = unpack(WAU[a]);                                                                                                             \
      FBN[a] = unpack(WBU[a]);                                                                                                             \
      _Pragma("unroll") for (int b = 0; b < 4; b++) acc[a][b] = mma(FA[a], FB[b], acc[a][b]);                                              \
      if constexpr (I8) {   /* 8 MFMAs, 28 unpack VALU, one DMA unit, two LDS reads */                                                     \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 4, 0); \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 4, 0); \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 4, 0); \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);                              \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);                              \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);                              \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);                              \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);                              \
      } else {                                                                                                                             \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 3, 0); \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 3, 0); \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 3, 0); \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);                                \
      }                                                                                                                                    \
      __builtin_amdgcn_sched_barrier(0);                                                                                                   \
    }                                                                                                                                      \
  }
  // two halves of the K range with the gang's second meeting between them (gm.ctr == nullptr: one pass); the stage loop itself stays one basic block
  const int nparts = gm.ctr ? gm.parts : 1;
  for (int part = 0; part < nparts; part++) {
  if (part > 0) {
    if (threadIdx.x == 0) {
      int *c = gm.ctr + (size_t)(part - 1) * gm.stride;
      __hip_atomic_fetch_add(c, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned long long tm = __builtin_amdgcn_s_memrealtime();
      while (__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < gm.target && __builtin_amdgcn_s_memrealtime() - tm < gm.ticks) __builtin_amdgcn_s_sleep(2);
    }
    __syncthreads();
  }
  const int s_lo = (int)((long)stages * part / nparts), s_hi = (int)((long)stages * (part + 1) / nparts);
  for (int s = s_lo; s < s_hi; s++) {
    // stage start: stage s+1 must have landed -- exactly (NB-2) stages' DMAs may stay in flight (one stage's 4 units are issued per stage,
    // always); this wave's reads of buffer s%NB were issued a K-step ago and are complete; after the barrier that buffer is refilled
    if (EXP != 2) {
      if (EXP != 3 && EXP != 6) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (NB - 2)) : "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (EXP != 4) __syncthreads();
    }
    const int dma_stage = min(s + NB, stages - 1), dma_buf = buf;
    buf = buf == NB - 1 ? 0 : buf + 1;
    const char *nxt = smem + buf * kXBufBytes;
    // t = 2s:   MFMAs F[0]; unpack W[1] (K-step 1 of this stage) -> F[1]; read K-step 0 of stage s+1 -> W[0]; refill buffer s%NB
    MXA_F4_KSTEP(fa0, fb0, wa1, wb1, fa1, fb1, wa0, wb0, nxt, true)
    // t = 2s+1: MFMAs F[1]; unpack W[0] (K-step 0 of stage s+1) -> F[0]; read K-step 1 of stage s+1 -> W[1]
    MXA_F4_KSTEP(fa1, fb1, wa0, wb0, fa0, fb0, wa1, wb1, nxt + 8, false)
  }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the redundant refills of the last stages have landed before the ring becomes scratch
#undef MXA_F4_KSTEP
  __syncthreads();   // all waves are done with the ring before it is reused as the epilogue scratch
  if (DIAG) {
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0 && diag) { diag[2 * tile_index] = t1 - t0; diag[2 * tile_index + 1] = r1 - r0; }
  }
  if constexpr (POST == kPostCounts) xprod_store_counts<AccT>(acc, reinterpret_cast<int *>(ans), t.w);   // ans = the count scratch, t.w = the tile's slot
  else xprod_store<AccT, POST>(acc, smem, wave, lane, wi, wj, i0, j0, t.z, n, ans, ld, c0, post);
}

template <bool DIAG, int EXP = 0, int POST = kPostNone>
__global__ void __launch_bounds__(256, 1)
k_crossprod_f4(const uint8_t *__restrict__ X, long nslabs, int stages, const int4 *__restrict__ tiles, long n, double *__restrict__ ans,
               long ld, long c0, unsigned long long *__restrict__ diag, XPost post) {
  const int4 t = tiles[blockIdx.x];
  if (t.z == 0) return;                         // padding entry of the XCD-aware tile order (whole workgroup, before any barrier)
  xprod_tile<DIAG, EXP, false, POST>(X, nslabs, stages, t, blockIdx.x, n, ans, ld, c0, diag, post);
}
template <bool DIAG, int POST = kPostNone>
__global__ void __launch_bounds__(256, 1)
k_crossprod_i8(const uint8_t *__restrict__ X, long nslabs, int stages, const int4 *__restrict__ tiles, long n, double *__restrict__ ans,
               long ld, long c0, unsigned long long *__restrict__ diag, XPost post) {
  const int4 t = tiles[blockIdx.x];
  if (t.z == 0) return;
  xprod_tile<DIAG, 0, true, POST>(X, nslabs, stages, t, blockIdx.x, n, ans, ld, c0, diag, post);
}

// ---- gang-synchronised persistent form (round 3) ------------------------------------------------------------------------------------------
// Every 256-row block of X is an operand of ~n/256 tiles, and the kernel above lets the tiles of an XCD drift apart along K (a finished workgroup is
// replaced at once, at its own time), so concurrent tiles rarely find each other's rows in the XCD's L2: the counters show 3.0 TB fetched per config-3
// launch (12.5 GB of operand, 243x), 3.7 TB/s next to a power-bound MFMA stream -- with every tile reading the SAME two blocks (results wrong) the
// clock rises from 2.01 to 2.19 GHz and the launch takes 7 % less.  Here ONE workgroup per CU stays resident and the P workgroups of an XCD advance
// through that XCD's tile list in GANGS: a workgroup that has finished claims the next slot (one returning atomic add) and waits until all P slots of
// the gang are claimed, i.e. until the whole XCD is ready, so that the gang's tiles -- 4 x 8 tiles of a super-tile: 12 row blocks for 32 tiles --
// start together and stream their operands in step (launches cut into waves of 256 tiles, the same synchronisation by other means, fetch 1.13 TB
// instead of 3.0).  Every wait is bounded by the clock (s_memrealtime): a workgroup that is not joined in time goes on alone, so the grid always
// drains whatever the hardware did with the workgroups (fewer CUs, another process on the chip); only the sharing is lost then.
// gang[0..7]: claim counters of the XCD lists, gang[8..15]: workgroups seen per XCD, gang[16]: workgroups seen in total (zeroed by the launcher).
constexpr int kGangCtrs = 17;
constexpr unsigned long long kGangJoinTicks = 10000;      // 100 us at the 100 MHz of s_memrealtime: ~4 % of a config-3 tile
constexpr unsigned long long kGangStartTicks = 200000;    // 2 ms for the whole grid to become resident
template <bool I8, int POST>
__global__ void __launch_bounds__(256, 1)
k_crossprod_gang(const uint8_t *__restrict__ X, long nslabs, int stages, const int4 *__restrict__ tiles, int slots_per_xcd, long n, double *__restrict__ ans,
                 long ld, long c0, XPost post, int *__restrict__ gang, unsigned join_ticks, int xcc_mask, int *__restrict__ mid, int mid_parts) {
  __shared__ int sh_val;
  const int xcc = hw_xcc_id() & xcc_mask;             // mask 7; the tests narrow it to emulate a chip that populates fewer XCDs (the other lists are then stolen)
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(gang + 8 + xcc, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(gang + 16, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__hip_atomic_load(gang + 16, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < (int)gridDim.x && __builtin_amdgcn_s_memrealtime() - t0 < kGangStartTicks)
      __builtin_amdgcn_s_sleep(16);
    sh_val = __hip_atomic_load(gang + 8 + xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const int P = max(1, sh_val);                       // workgroups of this XCD = gang size
  __syncthreads();
  __shared__ int sh_list, sh_own;
  int phase = 0;                                      // lane 0 only: 0 = the own XCD's list (in gangs), 1..7 = the other XCDs' lists once the own one is empty
  for (;;) {                                          // (no waiting there: correctness must not depend on which XCDs the hardware populated, e.g. a partitioned chip)
    if (threadIdx.x == 0) {
      int slot = -1, y = xcc;
      while (phase < 8) {
        y = (xcc + phase) & 7;
        slot = __hip_atomic_fetch_add(gang + y, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (slot < slots_per_xcd) break;
        slot = -1; phase++;
      }
      if (slot >= 0 && phase == 0) {
        const int target = min((slot / P + 1) * P, slots_per_xcd);
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__hip_atomic_load(gang + xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target && __builtin_amdgcn_s_memrealtime() - t0 < join_ticks)
          __builtin_amdgcn_s_sleep(4);
      }
      sh_val = slot; sh_list = y; sh_own = (slot >= 0 && phase == 0) ? 1 : 0;
    }
    __syncthreads();
    const int slot = __builtin_amdgcn_readfirstlane(sh_val), list = __builtin_amdgcn_readfirstlane(sh_list);
    if (slot < 0) break;                               // wave-uniform: every list is empty, the whole workgroup leaves
    const int4 tv = tiles[(size_t)8 * slot + list];
    const int4 t = make_int4(__builtin_amdgcn_readfirstlane(tv.x), __builtin_amdgcn_readfirstlane(tv.y), __builtin_amdgcn_readfirstlane(tv.z),
                              __builtin_amdgcn_readfirstlane(tv.w));   // scalar: the DMA bases live in SGPRs (w: the scratch slot of a count store)
    // second meeting point (mid != nullptr): the members of a gang of the own list meet again half way through the tile
    GangMid gm{nullptr, 0, 0, 1, 0};
    if (mid && __builtin_amdgcn_readfirstlane(sh_own)) {
      // (everything the stage loop's bounds depend on must be provably wave-uniform: the DMA bases and LDS addresses live in SGPRs)
      const int Pu = __builtin_amdgcn_readfirstlane(P), g = slot / Pu, members = __builtin_amdgcn_readfirstlane(min((g + 1) * Pu, slots_per_xcd) - g * Pu);
      const int idx = __builtin_amdgcn_readfirstlane(xcc * slots_per_xcd + g);
      // the meeting's wait: at most the join bound, and at most ~4 % of this tile (stages x 0.66 us at the FP4 rate = 66 ticks of 10 ns per stage)
      const unsigned mid_ticks = min(join_ticks, (unsigned)(2.64f * (float)stages));
      gm = GangMid{mid + idx, members, mid_ticks, mid_parts, 8 * slots_per_xcd};
      if (!t.z && threadIdx.x == 0)   // a padding entry never reaches the meetings: counted here
        for (int q = 0; q + 1 < mid_parts; q++) __hip_atomic_fetch_add(gm.ctr + (size_t)q * gm.stride, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (t.z) xprod_tile<false, 0, I8, POST>(X, nslabs, stages, t, 0, n, ans, ld, c0, nullptr, post, gm);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the stores of the epilogue: the DMA bookkeeping of the next tile starts from an empty counter
    __syncthreads();                                   // ... and the LDS scratch of the epilogue is free (sh_val / sh_list are rewritten only after this barrier)
  }
}

int launch_plink_lut(uint8_t *d, size_t nbytes, hipStream_t s) {
  const size_t nd = nbytes / 4;
  const int grid = (int)std::min<size_t>((nd + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(k_plink_lut, dim3(grid), dim3(256), 0, s, reinterpret_cast<uint32_t *>(d), nd);
  MXA_HIP(hipGetLastError());
  return 0;
}

// Order for the gang-synchronised kernel: the list is cut into GANGS of 32 tiles (the workgroups of an XCD) that are compact in the tile grid -- bands of 4
// tile rows, walked column by column, so a gang is 4 x 8 tiles = 12 row blocks (a little more where it meets the diagonal or the end of a band) -- and the
// gangs are dealt whole to the 8 XCD lists (neighbouring gangs of a band run on different XCDs at the same time and share the band's 4 row blocks through
// the Infinity Cache).  Gang boundaries stay aligned with multiples of 32 slots in every list; with the 8 x 8 super-tiles of round 2's order one
// partial super-tile (36 tiles on the diagonal) shifted every later gang of that list across two super-tile halves.
// Returns true when the list has the interleaved per-XCD form (list index = 8 * slot + xcd, padded with no-op entries {0,0,0,0}); false: too short, plain order.
static bool gang_order_tiles(std::vector<int4> &tiles) {
  constexpr size_t kGang = 32;
  if (tiles.size() < 8 * 64) return false;
  std::sort(tiles.begin(), tiles.end(), [](const int4 &a, const int4 &b) {
    if (a.x / 4 != b.x / 4) return a.x / 4 < b.x / 4;
    if (a.y != b.y) return a.y < b.y;
    return a.x < b.x;
  });
  std::vector<std::vector<int4>> per_xcd(8);
  size_t next = 0;
  for (size_t g0 = 0; g0 < tiles.size(); g0 += kGang) {
    std::vector<int4> &l = per_xcd[next];
    next = (next + 1) & 7;
    const size_t g1 = std::min(tiles.size(), g0 + kGang);
    l.insert(l.end(), tiles.begin() + (long)g0, tiles.begin() + (long)g1);
    l.resize((l.size() + kGang - 1) / kGang * kGang, make_int4(0, 0, 0, 0));      // only the very last gang is short
  }
  size_t longest = 0;
  for (auto &v : per_xcd) longest = std::max(longest, v.size());
  std::vector<int4> inter;
  inter.reserve(longest * 8);
  for (size_t slot = 0; slot < longest; slot++)
    for (int x = 0; x < 8; x++) inter.push_back(slot < per_xcd[x].size() ? per_xcd[x][slot] : make_int4(0, 0, 0, 0));
  tiles.swap(inter);
  return true;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static thread_local bool tl_xprod_shared_device = false;   // set by the panel workers of snp_multiply_gpu when several panels share a device
static std::mutex g_xprof_mutex;   // panels of one call run in several threads (MIRACULIX_NUM_GPUS): the profile counters are shared
namespace {
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
}  // namespace

// measured time of one 256 x 256 tile per K stage on one CU (FP4 / int8 MFMA): the estimates of the gang decision and of the ring
static double tile_stage_ms(bool f4) { return f4 ? 0.66e-3 : 1.0e-3; }

// the profile counts one launch per call, with the time between its two events
static hipError_t profile_launch(const XEvent &e0, const XEvent &e1) {
  float ms = 0.f;
  const hipError_t err = hipEventElapsedTime(&ms, e0.e, e1.e);
  if (err == hipSuccess) { std::lock_guard<std::mutex> lk(g_xprof_mutex); profile().launches += 1; profile().total_ms += ms; }
  return err;
}

// one launch of the kernel instantiation K with kF4Lds bytes of dynamic LDS: its attribute is set first (per device, once per instantiation)
template <auto K, typename... A>
static int launch_lds(dim3 grid, hipStream_t s, A... a) {
  static unsigned long long mask = 0;
  if (ensure_dyn_lds(reinterpret_cast<const void *>(K), kF4Lds, &mask)) return 1;
  hipLaunchKernelGGL(K, grid, dim3(256), kF4Lds, s, a...);
  MXA_HIP(hipGetLastError());
  return 0;
}
// the one-workgroup-per-tile instantiation of an engine
template <bool I8, bool DIAG, int POST> constexpr auto k_tiles = I8 ? &k_crossprod_i8<DIAG, POST> : &k_crossprod_f4<DIAG, 0, POST>;

// f(std::integral_constant<int, K>()) for every epilogue kind K
template <int... K, typename F>
static void for_each_post_kind(std::integer_sequence<int, K...>, F f) { (f(std::integral_constant<int, K>()), ...); }

// one launch over a tile list with either engine (f4: FP4 MFMA, else int8 MFMA); d_diag: in-kernel clocks of the DIAG instantiation
// gang_mid_capacity: ints available behind d_gang[32] for the per-gang counters of the second meeting point (0: none)
static int launch_tiles(const XGeom &g, bool f4, size_t ntiles, hipStream_t s, const uint8_t *d_X, const int4 *d_tiles, double *d_ans, long ld, long c0,
                        unsigned long long *d_diag, int post_kind, const XPost &post, int *d_gang, size_t gang_mid_capacity) {
  // gang-synchronised persistent form: needs the interleaved per-XCD lists (d_gang != nullptr) and is not instrumented (MXA_DIAG keeps the classic kernels)
  // It pays when the launch is long enough for the power limit to matter and a tile long enough to carry the meeting: config 3 -5 ... -8 %, 30 000 rows x
  // 500k -3.4 %, but K = 50 000 (0.26 ms per tile) +2 ... +8 % at 8 192 - 40 000 rows.  MXA_XPROD_GANG: 0 never, 1 (default) by this estimate, 2 whenever possible.
  static const int gang_on = [] { const char *e = getenv("MXA_XPROD_GANG"); return e ? atoi(e) : 1; }();
  int dev = 0, cus = 0;
  // not when this call is one of several panels computed side by side on ONE device (MIRACULIX_NUM_GPUS above the device count): the gang form wants one
  // workgroup per CU resident at once and would spend its 2 ms start-up wait on workgroups that cannot become resident beside the other panel's kernel
  if (gang_on && d_gang && !d_diag && ntiles % 8 == 0 && !(tl_xprod_shared_device && gang_on < 2)) {
    MXA_HIP(hipGetDevice(&dev));
    MXA_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  }
  const double est_ms = cus > 0 ? (double)g.stages * tile_stage_ms(f4) * ((double)ntiles / cus) : 0.0;
  const bool gang = cus > 0 && (gang_on >= 2 || (g.stages >= 1024 && est_ms >= 20.0));
  const int slots = (int)(ntiles / 8);
  int *d_mid = nullptr, mid_parts = 1, xcc_mask = 7;
  unsigned join_ticks = 0;
  if (gang) {
    static const int mask = [] { const char *e = getenv("MXA_XPROD_GANG_XCC_MASK"); return e ? atoi(e) & 7 : 7; }();
    static const unsigned ticks = [] { const char *e = getenv("MXA_XPROD_GANG_US"); return e ? (unsigned)std::max(0, atoi(e)) * 100u : (unsigned)kGangJoinTicks; }();
    xcc_mask = mask;
    join_ticks = ticks;
    MXA_HIP(hipMemsetAsync(d_gang, 0, sizeof(int) * kGangCtrs, s));
    // second meeting point: one counter per gang and XCD list, behind the 17 control counters when the caller's buffer has room for them
    // MXA_XPROD_GANG_MID = number of parts a tile's K range is cut into (meetings = parts - 1): 0 / 1 none, 2 (default) one meeting half way through.
    // The gang form is only taken for long tiles (stages >= 1024, i.e. K >= 131k: tiles of >= 0.7 ms), and the meeting's wait is bounded by 4 % of the tile.
    const char *e_mid = getenv("MXA_XPROD_GANG_MID");
    mid_parts = std::max(1, std::min(8, e_mid ? atoi(e_mid) : 2));
    if (mid_parts > 1 && gang_mid_capacity >= (size_t)8 * slots * (mid_parts - 1)) {
      d_mid = d_gang + 32;
      MXA_HIP(hipMemsetAsync(d_mid, 0, sizeof(int) * (size_t)8 * slots * (mid_parts - 1), s));
    }
  }
  const dim3 grid(gang ? (unsigned)std::max(8, std::min<int>(cus, (int)ntiles)) : (unsigned)ntiles);
  // the instantiation for (gang, engine, post_kind, diag); the GRM / LD maps never run in the diagnostic instantiations
  auto go = [&](auto i8, auto pk) {
    constexpr bool I8 = decltype(i8)::value;
    constexpr int POST = decltype(pk)::value;
    if (gang)
      return launch_lds<&k_crossprod_gang<I8, POST>>(grid, s, d_X, g.nslabs, g.stages, d_tiles, slots, g.rows, d_ans, ld, c0, post, d_gang, join_ticks, xcc_mask, d_mid, mid_parts);
    if (POST == kPostNone && d_diag) return launch_lds<k_tiles<I8, true, kPostNone>>(grid, s, d_X, g.nslabs, g.stages, d_tiles, g.rows, d_ans, ld, c0, d_diag, post);
    return launch_lds<k_tiles<I8, false, POST>>(grid, s, d_X, g.nslabs, g.stages, d_tiles, g.rows, d_ans, ld, c0, nullptr, post);
  };
  int rc = -1;
  for_each_post_kind(std::make_integer_sequence<int, kPostKinds>(), [&](auto pk) {
    if (post_kind == decltype(pk)::value) rc = f4 ? go(std::false_type(), pk) : go(std::true_type(), pk);
  });
  if (rc < 0) { set_error(1, "crossproduct: no epilogue kind %d", post_kind); return 1; }
  return rc;
}

// ---- tile lists.  Tile (i, j), i <= j, with flags bit 1: it writes its direct image M[J rows, I cols] (columns of tile i), bit 2: its mirror image
// M[I rows, J cols] (columns of tile j; never on the diagonal).
// The tiles that touch the column panel of tile columns [t0, t1); upper_only: the direct image only for j < t1 (rows on and above the panel's diagonal block).
static std::vector<int4> panel_tiles(int nb, int t0, int t1, bool upper_only) {
  std::vector<int4> tiles;
  for (int i = 0; i < nb; i++)
    for (int j = i; j < nb; j++) {
      int flags = 0;
      if (i >= t0 && i < t1 && (!upper_only || j < t1)) flags |= 1;
      if (j >= t0 && j < t1 && i != j) flags |= 2;
      if (flags) tiles.push_back(make_int4(i, j, flags, 0));
    }
  return tiles;
}
// The tile rows [i0, i1) of the upper triangle, both images of every tile.
static std::vector<int4> row_tiles(int nb, int i0, int i1) {
  std::vector<int4> tiles;
  for (int i = i0; i < i1; i++)
    for (int j = i; j < nb; j++) tiles.push_back(make_int4(i, j, i == j ? 1 : 3, 0));
  return tiles;
}

// The tiles of a window, tile row by tile row: (i, j), i <= j <= jmax[i] (LdWindow::plan: a band of ld_band_diagonals tile diagonals, or the reach of the
// tile row's last SNP).  A tile row is compact (neighbours that share row block i), which is what gang_order_tiles wants: a gang of 32 tiles is cut from
// four adjacent tile rows.
static std::vector<int4> window_tiles(const std::vector<int> &jmax) {
  std::vector<int4> tiles;
  for (int i = 0; i < (int)jmax.size(); i++)
    for (int j = i; j <= jmax[(size_t)i]; j++) tiles.push_back(make_int4(i, j, 1, 0));
  return tiles;
}

namespace {
// The tile lists of a call's chunks, uploaded once: chunk c is d_tiles[first[c], first[c + 1]), in the gang order where gang_order_tiles took it (xcd[c]).
// d_gang: the gangs' 32 control counters, then mid_cap ints for the counters of their meetings inside a tile, sized for the longest list.
struct XTiles {
  std::vector<int4> tiles;
  std::vector<size_t> first;
  std::vector<char> xcd;
  size_t mid_cap = 0;
  XBuf d_tiles, d_gang;
  int launch(int c, const XGeom &g, bool f4, hipStream_t s, const uint8_t *d_X, double *d_ans, long ld, long c0, unsigned long long *d_diag, int post_kind,
             const XPost &post) const {
    return launch_tiles(g, f4, first[(size_t)c + 1] - first[(size_t)c], s, d_X, (const int4 *)d_tiles.p + first[(size_t)c], d_ans, ld, c0, d_diag, post_kind,
                        post, xcd[(size_t)c] ? (int *)d_gang.p : nullptr, mid_cap);
  }
};
}  // namespace

static int upload_tiles(std::vector<std::vector<int4>> chunks, hipStream_t s, XTiles &t) {
  t.first.assign(chunks.size() + 1, 0);
  t.xcd.assign(chunks.size(), 0);
  for (size_t c = 0; c < chunks.size(); c++) {
    t.first[c] = t.tiles.size();
    t.xcd[c] = gang_order_tiles(chunks[c]);
    t.mid_cap = std::max(t.mid_cap, 7 * (chunks[c].size() + 64));      // >= 8 lists x slots per list x up to 7 meetings per tile
    t.tiles.insert(t.tiles.end(), chunks[c].begin(), chunks[c].end());
  }
  t.first.back() = t.tiles.size();
  if (t.d_tiles.alloc(t.tiles.size() * sizeof(int4)) || t.d_gang.alloc(sizeof(int) * (32 + t.mid_cap))) return 1;
  MXA_HIP(hipMemcpyAsync(t.d_tiles.p, t.tiles.data(), t.tiles.size() * sizeof(int4), hipMemcpyHostToDevice, s));
  return 0;
}

// X: device, tiled layout (rows padded to 256, K padded to 128 genotypes = nslabs slabs), zero padded.
// Columns [c_begin, c_end) of M = X X^T into d_ans (leading dimension ld; c_begin a multiple of the 256-row tile, c_end a multiple
// or the matrix end).  upper_only: only rows [0, c_end) are written -- everything above the panel's diagonal block and the block
// itself; rows >= c_end are left untouched.  The whole matrix is c_begin = 0, c_end = rows, ld = rows.
static int crossprod_device(const XGeom &g, const uint8_t *d_X, double *d_ans, hipStream_t s, long c_begin, long c_end, bool upper_only, long ld, bool f4,
                            int post_kind, const XPost &post) {
  XTiles t;
  if (upload_tiles({panel_tiles(g.nb, (int)(c_begin / kXT), (int)((c_end + kXT - 1) / kXT), upper_only)}, s, t)) return 1;
  const size_t ntiles = t.tiles.size();
  XEvent e0, e1;
  if (e0.create() || e1.create()) return 1;
  XBuf d_diag;
  const bool diag_on = getenv("MXA_DIAG") != nullptr;
  if (diag_on && d_diag.alloc(16 * ntiles)) return 1;
  MXA_HIP(hipEventRecord(e0.e, s));
  if (t.launch(0, g, f4, s, d_X, d_ans, ld, c_begin, (unsigned long long *)d_diag.p, post_kind, post)) return 1;
  MXA_HIP(hipEventRecord(e1.e, s));
  MXA_HIP(hipStreamSynchronize(s));   // tiles vector / d_tiles lifetime
  if (diag_on) {   // diagnostic instantiation: in-kernel clock and cycles per stage
    std::vector<unsigned long long> hd(2 * ntiles);
    MXA_HIP(hipMemcpy(hd.data(), d_diag.p, 16 * ntiles, hipMemcpyDeviceToHost));
    std::vector<double> ghz, cyc;
    for (size_t i = 0; i < ntiles; i++) if (t.tiles[i].z && hd[2 * i + 1]) { ghz.push_back((double)hd[2 * i] / (double)hd[2 * i + 1] * 0.1); cyc.push_back((double)hd[2 * i] / g.stages); }
    std::sort(ghz.begin(), ghz.end()); std::sort(cyc.begin(), cyc.end());
    if (!ghz.empty()) printf("MXA_DIAG %s: %zu tiles, in-kernel clock median %.3f GHz (min %.3f max %.3f); shader cycles per stage median %.0f (ideal %d)\n",
                             f4 ? "k_crossprod_f4" : "k_crossprod_i8", ntiles, ghz[ghz.size() / 2], ghz.front(), ghz.back(), cyc[cyc.size() / 2], f4 ? 1024 : 2048);
  }
  MXA_HIP(profile_launch(e0, e1));
  return 0;
}

// Whole matrix for a HOST result, in chunks of ~1 GiB column slabs: chunk c holds columns [256 w c, 256 w (c + 1)) of M, and four helper threads copy each
// finished chunk to the host, each on its own non-blocking stream, while the next chunk computes (at config 3 the 80 GB device-to-host copy is as long
// as the compute).  Two forms:
//  - into d_ans, the n x n device buffer: chunk c is the tile rows [w c, w (c + 1)) (all j >= i).  Tile (i, j) stores M[J rows, I cols] and M[I rows, J cols],
//    so once every chunk up to tile row i1 has run, columns [0, 256*i1) of M are final.
//  - ring (round 4): no device copy of the whole matrix.  Its hipMalloc (80 GB at config 3) takes anything from nothing to 4.6 s on this pool (the phase
//    clock of crossprod_any, profiles/r04_crossprod_host_*.txt: that -- not a copy scheme -- was round 3's unexplained "one call in 24 takes 4-5 s"), and
//    the result could never exceed HBM.  Chunk c is the column panel of mxa_snp_multiply_panel (every tile (i, j >= i) that touches it), computed into
//    slot c % 3 of a RING of device buffers.  Every off-diagonal tile is computed twice (once per image): twice the arithmetic of the triangular
//    launch -- taken only where the call is bound by the copy anyway (crossprod_any compares the two estimates).
static int crossprod_slabs(const XGeom &g, const uint8_t *d_X, double *d_ans, double *h_ans, hipStream_t s, bool f4, int post_kind, const XPost &post,
                           bool ring, HostPrefault &pf) {
  const long rows = g.rows;
  const char *slab_env = getenv("MXA_XPROD_SLAB_MB");                                        // tests use small slabs
  const long slab_bytes = (slab_env && atol(slab_env) > 0 ? atol(slab_env) : 1024L) << 20;
  const int w = (int)std::max<long>(1, slab_bytes / (rows * 8 * kXT));                        // tile rows or tile columns per chunk
  const int nchunks = (g.nb + w - 1) / w;
  constexpr int kRing = 3, kCopiers = 4;
  XBuf slot[kRing];
  if (ring)
    for (auto &r : slot) if (r.alloc((size_t)rows * (size_t)std::min<long>(rows, (long)w * kXT) * sizeof(double))) return 1;
  std::vector<std::vector<int4>> chunks;
  for (int c = 0; c < nchunks; c++) chunks.push_back(ring ? panel_tiles(g.nb, c * w, std::min(g.nb, (c + 1) * w), false) : row_tiles(g.nb, c * w, std::min(g.nb, (c + 1) * w)));
  XTiles t;
  if (upload_tiles(std::move(chunks), s, t)) return 1;
  // chunk c: its first column, and the output its launch writes -- base pointer and the column held there first
  auto col0 = [&](int c) { return std::min<long>(rows, (long)c * w * kXT); };
  auto out = [&](int c) { return ring ? std::make_pair((double *)slot[c % kRing].p, col0(c)) : std::make_pair(d_ans, 0L); };
  std::vector<XEvent> ev((size_t)nchunks);
  int dev = 0;
  MXA_HIP(hipGetDevice(&dev));
  for (auto &e : ev) if (e.create(hipEventDisableTiming)) return 1;
  XEvent e0, e1;
  if (e0.create() || e1.create()) return 1;
  std::atomic<int> launched{0}, copy_err{0};
  std::atomic<bool> abort_copy{false};
  std::vector<std::atomic<int>> copied((size_t)nchunks);   // copiers done with chunk c: its ring slot is free once all are
  for (auto &c : copied) c.store(0);
  // a copy into pageable memory is staged by the runtime and bound by one host thread's memcpy (~17 GB/s measured): several
  // copier threads, each with its own stream and its own share of every slab, run those memcpys side by side
  XStream cs[kCopiers];
  for (auto &c : cs) if (c.create(hipStreamNonBlocking)) return 1;
  // where the host time of a call goes, per copier: waiting for a slab to be computed, and inside the copies; the slowest single copy with its
  // slab (a stall shows up there).  Printed under PRINT_LEVEL / print_details (debug_info) together with the prefault of the destination.
  struct CopierLog { double wait_s = 0, copy_s = 0, worst_s = 0; int worst_slab = -1; size_t bytes = 0; };
  CopierLog clog[kCopiers];
  const auto t_call = std::chrono::steady_clock::now();
  auto since = [&](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count(); };
  auto copy_loop = [&](int th) {
    if (hipSetDevice(dev) != hipSuccess) { copy_err = 1; abort_copy = true; return; }
    for (int c = 0; c < nchunks; c++) {
      const auto tw = std::chrono::steady_clock::now();
      while (launched.load() <= c) { if (abort_copy.load()) return; std::this_thread::yield(); }
      if (hipEventSynchronize(ev[c].e) != hipSuccess) { copy_err = 1; abort_copy = true; return; }
      clog[th].wait_s += since(tw);
      const long width = col0(c + 1) - col0(c), a = col0(c) + width * th / kCopiers, b = col0(c) + width * (th + 1) / kCopiers;   // this copier's columns
      if (b > a) {
        const auto [o, oc0] = out(c);
        const size_t cnt = (size_t)(b - a) * rows;
        double *dst = h_ans + (size_t)a * rows;
        const auto tp = std::chrono::steady_clock::now();
        pf.wait_for(dst + cnt);   // the destination pages exist: no faults inside the copy
        clog[th].wait_s += since(tp);
        const auto tc = std::chrono::steady_clock::now();
        if (hipMemcpyAsync(dst, o + (size_t)(a - oc0) * rows, cnt * sizeof(double), hipMemcpyDeviceToHost, cs[th].s) != hipSuccess ||
            hipStreamSynchronize(cs[th].s) != hipSuccess) { copy_err = 1; abort_copy = true; return; }
        const double dt = since(tc);
        clog[th].copy_s += dt; clog[th].bytes += cnt * sizeof(double);
        if (dt > clog[th].worst_s) { clog[th].worst_s = dt; clog[th].worst_slab = c; }
      }
      copied[(size_t)c].fetch_add(1);
    }
  };
  // the ring's destination pages are populated from here on: every device buffer, stream and event of the call exists (mxa_hostmem.h; the other form's
  // population started when crossprod_any had allocated d_ans)
  if (ring) pf.start(h_ans, (size_t)rows * (size_t)rows * sizeof(double));
  std::vector<std::thread> copiers;
  for (int th = 0; th < kCopiers; th++) copiers.emplace_back(copy_loop, th);
  int rc = 0;
  double t_wait_slot = 0.0;
  if (hipEventRecord(e0.e, s) != hipSuccess) rc = 1;
  for (int c = 0; c < nchunks && !rc; c++) {
    if (ring && c >= kRing) {   // the slot is free once all copiers have taken chunk c - kRing out of it
      const auto tw = std::chrono::steady_clock::now();
      while (copied[(size_t)(c - kRing)].load() < kCopiers) { if (abort_copy.load()) { rc = 1; break; } std::this_thread::yield(); }
      t_wait_slot += since(tw);
      if (rc) break;
    }
    const auto [o, oc0] = out(c);
    if (t.launch(c, g, f4, s, d_X, o, rows, oc0, nullptr, post_kind, post) || hipEventRecord(ev[c].e, s) != hipSuccess) { rc = 1; break; }
    launched.store(c + 1);
  }
  if (rc) abort_copy = true;
  if (!rc && hipEventRecord(e1.e, s) != hipSuccess) rc = 1;
  const double t_launched = since(t_call);
  for (auto &th : copiers) th.join();
  if (hipStreamSynchronize(s) != hipSuccess) rc = 1;
  char form[32] = "";
  if (ring) snprintf(form, sizeof form, " (ring of %d slabs)", kRing);
  for (int th = 0; th < kCopiers; th++)
    debug_info("crossproduct host result%s: copier %d waited %.3f s for slabs, copied %.2f GB in %.3f s (%.1f GB/s), slowest single copy %.3f s (slab %d of %d)", form, th,
               clog[th].wait_s, clog[th].bytes * 1e-9, clog[th].copy_s, clog[th].copy_s > 0 ? clog[th].bytes * 1e-9 / clog[th].copy_s : 0.0, clog[th].worst_s,
               clog[th].worst_slab, nchunks);
  if (ring) debug_info("crossproduct host result (ring): %d slab launches enqueued after %.3f s (%.3f s of it waiting for a free slot), all copies done after %.3f s", nchunks, t_launched, t_wait_slot, since(t_call));
  else debug_info("crossproduct host result: %d slab launches enqueued after %.3f s, all copies done after %.3f s", nchunks, t_launched, since(t_call));
  if (!rc && !copy_err.load()) (void)profile_launch(e0, e1);
  if (rc || copy_err.load()) { set_error(13, "snp_multiply_gpu: pipelined device-to-host copy of the result failed"); return 1; }
  return 0;
}

// ---- GRM / LD post-processing on the device (reference: host BLAS in src/bindings/Julia/crossproduct.jl:83-152, maths docs/grm.md)
// column sums of the symmetric n x n matrix, fixed-order tree per column
__global__ void __launch_bounds__(256) k_sym_colsum(const double *__restrict__ M, long n, double *__restrict__ cs) {
  const long j = blockIdx.x;
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) s += M[(size_t)j * n + i];
  __shared__ double sh[256];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) { if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w]; __syncthreads(); }
  if (threadIdx.x == 0) cs[j] = sh[0];
}
// out[0] = sum_i v[i] * (w ? (1 - w[i]) * 2 : 1)   (single block, fixed order)
__global__ void __launch_bounds__(1024) k_vec_reduce(const double *__restrict__ v, long n, int mode, double *__restrict__ out) {
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 1024) s += mode ? 2.0 * v[i] * (1.0 - v[i]) : v[i];
  __shared__ double sh[1024];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) { if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w]; __syncthreads(); }
  if (threadIdx.x == 0) out[0] = sh[0];
}
// G = (M - cs 1^T / n - 1 cs^T / n + total / n^2) / c          (crossproduct.jl:96-107)
__global__ void __launch_bounds__(256) k_grm_update(double *__restrict__ M, long n, const double *__restrict__ cs, const double *__restrict__ total,
                                                    const double *__restrict__ c, int do_scale) {
  const long j = blockIdx.x;                               // column: gridDim.x may exceed 65535, gridDim.y may not
  const long i = (long)blockIdx.y * 256 + threadIdx.x;
  if (i >= n) return;
  const double inv_n = 1.0 / (double)n;
  M[(size_t)j * n + i] = grm_map(M[(size_t)j * n + i], cs[i], cs[j], inv_n, total[0] / ((double)n * (double)n), do_scale ? 1.0 / c[0] : 1.0, do_scale);
}
// LD: M <- M - 4 * indiv * f f^T ; sigma = sqrt(diag M) ; M <- M / sigma sigma^T      (crossproduct.jl:139-149)
__global__ void __launch_bounds__(256) k_ld_center(double *__restrict__ M, long n, const double *__restrict__ f, double four_indiv) {
  const long j = blockIdx.x;
  const long i = (long)blockIdx.y * 256 + threadIdx.x;
  if (i >= n) return;
  M[(size_t)j * n + i] = ld_center_map(M[(size_t)j * n + i], f[i], f[j], four_indiv);
}
__global__ void __launch_bounds__(256) k_diag_sqrt(const double *__restrict__ M, long n, double *__restrict__ sigma) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) sigma[i] = 1.0 / sqrt(M[(size_t)i * n + i]);   // reciprocal: ld_scale_map multiplies
}
__global__ void __launch_bounds__(256) k_ld_scale(double *__restrict__ M, long n, const double *__restrict__ sigma) {
  const long j = blockIdx.x;
  const long i = (long)blockIdx.y * 256 + threadIdx.x;
  if (i >= n) return;
  M[(size_t)j * n + i] = ld_scale_map(M[(size_t)j * n + i], sigma[i], sigma[j]);
}

// ---- what the fused map needs, from the staged 2-bit matrix X (tiled layout, values 0..3) instead of from the 8 n^2-byte result ----------------
// t[s] = sum over all rows of x[r][s] (int32: <= 3 rows).  One block per slab of 128 genotypes walks all row tiles; thread tid reads dword
// it * 256 + tid of every 8-KiB tile (lane-linear), i.e. always dword `tid & 7` of a row piece: 16 fixed genotype columns per thread.  SWAR byte
// counters (4 fields per register), flushed to 16 int32 counters before they can overflow; fixed-order reduction over the 32 threads of a column group.
__global__ void __launch_bounds__(256) k_x_colsum(const uint8_t *__restrict__ X, long nslabs, long ntiles, int *__restrict__ t) {
  const long slab = blockIdx.x;
  const int tid = threadIdx.x;
  uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  int cnt[16];
#pragma unroll
  for (int f = 0; f < 16; f++) cnt[f] = 0;
  auto flush = [&]() {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      cnt[4 * q + 0] += (int)((a0 >> (8 * q)) & 255u); cnt[4 * q + 1] += (int)((a1 >> (8 * q)) & 255u);
      cnt[4 * q + 2] += (int)((a2 >> (8 * q)) & 255u); cnt[4 * q + 3] += (int)((a3 >> (8 * q)) & 255u);
    }
    a0 = a1 = a2 = a3 = 0;
  };
  int pend = 0;
  for (long rt = 0; rt < ntiles; rt++) {
    const uint32_t *tile = reinterpret_cast<const uint32_t *>(X + ((size_t)rt * nslabs + (size_t)slab) * kTileBytes);
#pragma unroll
    for (int it = 0; it < 8; it++) {
      const uint32_t w = tile[it * 256 + tid];
      a0 += w & 0x03030303u; a1 += (w >> 2) & 0x03030303u; a2 += (w >> 4) & 0x03030303u; a3 += (w >> 6) & 0x03030303u;
    }
    pend += 8;                                   // every byte counter grew by at most 3 * 8
    if (pend + 8 > 85) { flush(); pend = 0; }    // 85 * 3 = 255
  }
  flush();
  __shared__ int sh[256][17];
#pragma unroll
  for (int f = 0; f < 16; f++) sh[tid][f] = cnt[f];
  __syncthreads();
  if (tid < 128) {
    const int part = tid >> 4, f = tid & 15;     // genotype part * 16 + f of the slab = field f of dword `part` of the row piece
    int sum = 0;
    for (int g = 0; g < 32; g++) sum += sh[g * 8 + part][f];
    t[slab * 128 + tid] = sum;
  }
}
// per row r: cs[r] += sum_s x[r][s] * t[s]  (WANT_CS;  = column sum r of M = X X^T)  and / or  dg[r] += sum_s x[r][s]^2  (WANT_DG; = M[r][r]).
// Grid (row tiles, K chunks); thread = row of the tile, reading its 32-byte piece of every slab of the chunk (a wave reads 2 KiB contiguous);
// the t values of a slab are broadcast from LDS.  Exact integers: 32 bits within a dword of 16 fields (rows < 29.8 M: kXFusedMaxRows), 64 bits beyond, 64-bit atomics
// across the chunks (integer addition: order-independent).
template <bool WANT_CS, bool WANT_DG>
__global__ void __launch_bounds__(256) k_x_rowstats(const uint8_t *__restrict__ X, long nslabs, long slabs_per_chunk, const int *__restrict__ t,
                                                    unsigned long long *__restrict__ cs, unsigned long long *__restrict__ dg) {
  const long rt = blockIdx.x;
  const long s0 = (long)blockIdx.y * slabs_per_chunk, s1 = min(nslabs, s0 + slabs_per_chunk);
  const int tid = threadIdx.x;
  __shared__ int tsh[128];
  unsigned long long acc_cs = 0, acc_dg = 0;
  for (long sl = s0; sl < s1; sl++) {
    if (WANT_CS) {
      __syncthreads();
      if (tid < 128) tsh[tid] = t[sl * 128 + tid];
      __syncthreads();
    }
    const uint4 *pp = reinterpret_cast<const uint4 *>(X + ((size_t)rt * nslabs + (size_t)sl) * kTileBytes + (size_t)tid * kSlabBytes);
    const uint4 q0 = pp[0], q1 = pp[1];
    const uint32_t w[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    unsigned long long part_cs = 0;
    uint32_t part_dg = 0;
#pragma unroll
    for (int d = 0; d < 8; d++) {
      if (WANT_CS) {   // 32 bits hold the 16 fields of one dword (16 * 3 * 3 rows < 2^32 for rows < 29.8 M, guarded by the caller); across dwords 64 bits
        uint32_t pd = 0;
#pragma unroll
        for (int f = 0; f < 16; f++) pd += ((w[d] >> (2 * f)) & 3u) * (uint32_t)tsh[d * 16 + f];
        part_cs += pd;
      }
      if (WANT_DG) {   // x^2 = 1, 4, 9 for x = 1, 2, 3: three bit counts
        const uint32_t L = w[d] & 0x55555555u, H = (w[d] >> 1) & 0x55555555u;
        part_dg += (uint32_t)__popc(L & ~H) + 4u * (uint32_t)__popc(H & ~L) + 9u * (uint32_t)__popc(H & L);
      }
    }
    acc_cs += part_cs; acc_dg += part_dg;
  }
  const long r = rt * kTileRows + tid;
  if (WANT_CS && acc_cs) atomicAdd(cs + r, acc_cs);
  if (WANT_DG && acc_dg) atomicAdd(dg + r, acc_dg);
}
// u64 -> double (exact below 2^53), or the reciprocal LD sigma: 1 / sqrt(M_ii - 4 indiv f_i^2) exactly as k_ld_center + k_diag_sqrt form it
__global__ void __launch_bounds__(256) k_x_finish_stats(const unsigned long long *__restrict__ in, long n, const double *__restrict__ f, double four_indiv, double *__restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double v = (double)in[i];
  out[i] = f ? 1.0 / sqrt(ld_center_map(v, f[i], f[i], four_indiv)) : v;
}

// post: kPostNone, kPostGrm (do_scale as given, f = allele frequencies of length k), kPostLd (f of length rows, k = number of individuals)
static int postprocess_device(double *d_M, long rows, long k, int post, int do_scale, const double *d_f, hipStream_t s) {
  if (post == kPostNone) return 0;
  XBuf tmp_buf;
  if (tmp_buf.alloc(sizeof(double) * (size_t)(rows + 4))) return 1;
  double *tmp = (double *)tmp_buf.p;
  dim3 g2((unsigned)rows, (unsigned)((rows + 255) / 256));   // x = column (unbounded), y = row chunk (<= 65535)
  if (post == kPostGrm) {
    hipLaunchKernelGGL(k_sym_colsum, dim3((unsigned)rows), dim3(256), 0, s, d_M, rows, tmp);
    hipLaunchKernelGGL(k_vec_reduce, dim3(1), dim3(1024), 0, s, tmp, rows, 0, tmp + rows);
    if (do_scale) hipLaunchKernelGGL(k_vec_reduce, dim3(1), dim3(1024), 0, s, d_f, k, 1, tmp + rows + 1);
    hipLaunchKernelGGL(k_grm_update, g2, dim3(256), 0, s, d_M, rows, tmp, tmp + rows, tmp + rows + 1, do_scale);
  } else {
    hipLaunchKernelGGL(k_ld_center, g2, dim3(256), 0, s, d_M, rows, d_f, 4.0 * (double)k);
    hipLaunchKernelGGL(k_diag_sqrt, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, d_M, rows, tmp);
    hipLaunchKernelGGL(k_ld_scale, g2, dim3(256), 0, s, d_M, rows, tmp);
  }
  MXA_HIP(hipGetLastError());
  MXA_HIP(hipStreamSynchronize(s));
  return 0;
}

// X (rows of row_bytes packed bytes, in device or host memory) -> d_X, zeroed first, in the tiled layout (k_xstage; is_plink: the reference's table);
// *d_has3 = 1 when a staged field holds the value 3.  Host rows go through `bounce` (<= 256 MiB: kept by the caller, the pre-flight counts it).
// planes_indiv > 0: the three planes Z, M, A of the pairwise-complete LD instead (k_xstage_planes; d_X holds 3 * rows_pad rows, *d_has3 = a missing code occurs).
// mask_fields > 0: a row holds that many fields, its padding bits are staged as 00 (the GRM / LD entries); 0: the bytes as stored (the plain crossproduct).
static int stage_operand(const unsigned char *snp_matrix, bool in_dev, long row_bytes, bool is_plink, const XGeom &g, uint8_t *d_X, int *d_has3, XBuf &bounce,
                         hipStream_t s, long planes_indiv = 0, long mask_fields = 0) {
  const long rows = g.rows;
  const size_t plane_bytes = (size_t)g.rows_pad() * g.pitch();
  MXA_HIP(hipMemsetAsync(d_X, 0, plane_bytes * (planes_indiv > 0 ? 3 : 1), s));
  MXA_HIP(hipMemsetAsync(d_has3, 0, sizeof(int), s));
  // rows [r0, r0 + nr) of src (pitch row_bytes) into the staged operand
  auto stage = [&](const uint8_t *src, long r0, long nr) {
    const dim3 grid((unsigned)std::min<long>((nr * ((row_bytes + 3) / 4) + 255) / 256, 8192));
    if (planes_indiv > 0) hipLaunchKernelGGL(k_xstage_planes, grid, dim3(256), 0, s, src, (size_t)row_bytes, row_bytes, nr, planes_indiv, d_X, g.nslabs, plane_bytes, r0, d_has3);
    else hipLaunchKernelGGL(k_xstage, grid, dim3(256), 0, s, src, (size_t)row_bytes, row_bytes, nr, d_X, g.nslabs, r0, is_plink ? 1 : 0, d_has3, mask_fields);
  };
  if (in_dev) {
    stage(snp_matrix, 0L, rows);
    MXA_HIP(hipGetLastError());
    return 0;
  }
  long chunk_rows = std::max<long>(1, (long)(((size_t)256 << 20) / (size_t)row_bytes));
  chunk_rows = std::min(chunk_rows, rows);
  if (bounce.alloc((size_t)chunk_rows * row_bytes)) return 1;
  for (long r0 = 0; r0 < rows; r0 += chunk_rows) {
    const long nr = std::min(chunk_rows, rows - r0);
    MXA_HIP(hipMemcpyAsync(bounce.p, snp_matrix + (size_t)r0 * row_bytes, (size_t)nr * row_bytes, hipMemcpyHostToDevice, s));
    stage((const uint8_t *)bounce.p, r0, nr);
    MXA_HIP(hipGetLastError());
    MXA_HIP(hipStreamSynchronize(s));
  }
  return 0;
}

// grid of the per-row passes over the staged operand (k_x_rowstats, k_pw_rowsums): (row tiles, K chunks of *spc slabs each), ~1024 blocks at least
static dim3 rowstats_grid(const XGeom &g, long *spc) {
  const long chunks = std::max<long>(1, std::min<long>(g.nslabs, (1024 + g.nb - 1) / g.nb));
  *spc = (g.nslabs + chunks - 1) / chunks;
  return dim3((unsigned)g.nb, (unsigned)((g.nslabs + *spc - 1) / *spc));
}

// What the GRM (kPostGrm) / LD (kPostLd) map fused into the epilogue needs, from the staged 2-bit matrix: ~2 passes over rows * k / 4 bytes instead of 3 over
// 8 * rows^2.  xp points into st[2]; st[0..2] are kept by the caller until the product has run.
static int fused_post_stats(const XGeom &g, const uint8_t *d_X, long k, int post, int do_scale, const double *d_f, XBuf (&st)[3], hipStream_t s, XPost &xp) {
  const long rows = g.rows, rows_pad = g.rows_pad(), nslabs = g.nslabs, ntiles = g.nb;
  if (st[0].alloc(sizeof(int) * (size_t)nslabs * 128) || st[1].alloc(sizeof(unsigned long long) * (size_t)rows_pad) || st[2].alloc(sizeof(double) * (size_t)(rows_pad + 4))) return 1;
  MXA_HIP(hipMemsetAsync(st[1].p, 0, sizeof(unsigned long long) * (size_t)rows_pad, s));
  int *t = (int *)st[0].p;
  unsigned long long *raw = (unsigned long long *)st[1].p;
  double *out = (double *)st[2].p;
  long spc = 0;
  const dim3 g_rows = rowstats_grid(g, &spc);
  const unsigned g_fin = (unsigned)((rows + 255) / 256);
  if (post == kPostGrm) {
    hipLaunchKernelGGL(k_x_colsum, dim3((unsigned)nslabs), dim3(256), 0, s, d_X, nslabs, ntiles, t);
    hipLaunchKernelGGL((k_x_rowstats<true, false>), g_rows, dim3(256), 0, s, d_X, nslabs, spc, (const int *)t, raw, (unsigned long long *)nullptr);
    hipLaunchKernelGGL(k_x_finish_stats, dim3(g_fin), dim3(256), 0, s, raw, rows, (const double *)nullptr, 0.0, out);
    hipLaunchKernelGGL(k_vec_reduce, dim3(1), dim3(1024), 0, s, out, rows, 0, out + rows_pad);
    if (do_scale) hipLaunchKernelGGL(k_vec_reduce, dim3(1), dim3(1024), 0, s, d_f, k, 1, out + rows_pad + 1);
    xp.u = out; xp.scal = out + rows_pad; xp.a = 1.0 / (double)rows; xp.do_scale = do_scale;
  } else {
    hipLaunchKernelGGL((k_x_rowstats<false, true>), g_rows, dim3(256), 0, s, d_X, nslabs, spc, (const int *)nullptr, (unsigned long long *)nullptr, raw);
    hipLaunchKernelGGL(k_x_finish_stats, dim3(g_fin), dim3(256), 0, s, raw, rows, d_f, 4.0 * (double)k, out);
    xp.u = d_f; xp.w = out; xp.a = 4.0 * (double)k;
  }
  MXA_HIP(hipGetLastError());
  return 0;
}

constexpr long kXFusedMaxRows = 29000000L;   // k_x_rowstats: 16 * 3 * (3 rows) must fit 32 bits

// engine: FP4 while the fp32 accumulator is provably exact (sum z z' < 2^24), int8 beyond (MXA_XPROD_ENGINE=i8 forces int8, for A/B runs)
static int pick_engine(const int *d_has3, long k, hipStream_t s, bool &f4) {
  int has3 = 1;
  MXA_HIP(hipMemcpyAsync(&has3, d_has3, sizeof(int), hipMemcpyDeviceToHost, s));
  MXA_HIP(hipStreamSynchronize(s));
  f4 = has3 ? 9 * k < (1L << 24) : 4 * k < (1L << 24);
  if (const char *e = getenv("MXA_XPROD_ENGINE")) { if (!strcmp(e, "i8")) f4 = false; }
  return 0;
}

static int crossprod_any(const unsigned char *snp_matrix, long k, long rows, double *ans, bool is_plink, int post = kPostNone, int do_scale = 0,
                         const double *freq = nullptr, long c_begin = 0, long c_end = -1, bool upper_only = false, long ld = -1, int device = -1) {
  if (c_end < 0) c_end = rows;
  if (ld < 0) ld = rows;
  if (!snp_matrix || !ans || k <= 0 || rows <= 0) { set_error(1, "snp_multiply_gpu: bad arguments"); return 1; }
  if (device >= 0) MXA_HIP(hipSetDevice(device));
  else if (select_device() < 0) return 1;   // HIP_DEVICE / CUDA_DEVICE with the range check; GPU-only
  const XGeom g(k, rows);
  const long row_bytes = (k + 3) / 4;
  const bool in_dev = ptr_location(snp_matrix, nullptr) == 1, out_dev = ptr_location(ans, nullptr) == 1;
  if (c_begin < 0 || c_begin >= c_end || c_end > rows || c_begin % kXT != 0 || (c_end % kXT != 0 && c_end != rows) || ld < (upper_only ? c_end : rows)) {
    set_error(1, "crossproduct panel: need 0 <= col_begin < col_end <= n, col_begin %% %d == 0, col_end %% %d == 0 or col_end == n, ld >= rows written", kXT, kXT);
    return 1;
  }
  const bool whole = c_begin == 0 && c_end == rows && !upper_only;
  // a whole-matrix host result leaves slab by slab (crossprod_slabs) unless MXA_XPROD_NO_PIPELINE asks for one copy at the end
  const bool pipelined = !out_dev && whole && ld == rows && !getenv("MXA_XPROD_NO_PIPELINE");
  const char *e_fused = getenv("MXA_XPROD_FUSED_POST");   // read per call (tests compare both paths bit for bit)
  const bool fused_on = !e_fused || atoi(e_fused) != 0;
  const size_t xbytes = (size_t)g.rows_pad() * g.pitch(), abytes = (size_t)ld * (size_t)(c_end - c_begin) * sizeof(double);
  size_t free_b = 0, total_b = 0;
  MXA_HIP(hipMemGetInfo(&free_b, &total_b));
  // a pipelined result can leave through the ring of three ~1 GiB slabs: the n x n device copy is then not needed
  const size_t out_need = out_dev ? 0 : (pipelined ? std::min<size_t>(abytes, (size_t)3400 << 20) : abytes);
  const size_t need = xbytes + out_need + (in_dev ? 0 : std::min<size_t>((size_t)rows * row_bytes, (size_t)256 << 20));
  if (need > free_b) { set_error(12, "snp_multiply_gpu: not enough device memory: required %zu GB, free %zu GB", need >> 30, free_b >> 30); return 1; }
  // a host result in fresh memory (crossproduct.jl:56 `M = zeros(...)`): its pages are populated in the background while the tiles are computed, so that
  // the copies do not pay the first-touch faults (mxa_hostmem.h).  Joined when this returns.
  // Started only AFTER the operand has been staged and EVERY device buffer of the call has been allocated: twelve threads inside madvise slow a concurrent
  // hipMalloc (12.5 GB: 1.2-1.3 s instead of < 0.06 s; the 3 GiB ring: 1.7 s) and the staged pageable upload (1.55 s instead of 0.24 s) by far more than
  // the head start is worth (profiles/r04_crossprod_host_abi_c3.txt).
  HostPrefault prefault;
  struct PrefaultReport {
    HostPrefault &p;
    ~PrefaultReport() {
      p.join();
      if (p.threads()) debug_info("host result: %.2f GB of destination pages populated in the background by %d threads in %.3f s%s", p.populated() * 1e-9, p.threads(), p.seconds(),
                                  p.unsupported() ? " (MADV_POPULATE_WRITE not supported by this kernel: first-touch faults stay in the copies)" : "");
    }
  } prefault_report{prefault};
  // phase clock of a call with a host operand (debug_info under PRINT_LEVEL): where the wall time of the plain ABI goes
  struct PhaseClock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), last = t0;
    bool on;
    explicit PhaseClock(bool o) : on(o) {}
    void mark(const char *what) {
      if (!on) return;
      const auto now = std::chrono::steady_clock::now();
      debug_info("crossproduct call: %-34s %.3f s (at %.3f s)", what, std::chrono::duration<double>(now - last).count(), std::chrono::duration<double>(now - t0).count());
      last = now;
    }
  } clk(true);   // (round 5: for device operands too -- the operand is re-tiled into a buffer allocated per call, and hipMalloc of 12.5 GB takes 0-1.3 s on this pool)
  XStream st;
  if (st.create(hipStreamDefault)) return 1;   // blocking: ordered against the caller's default-stream work
  hipStream_t s = st.s;
  XBuf d_X, bounce, d_out, d_flag, f_tmp;
  if (d_X.alloc(xbytes) || d_flag.alloc(sizeof(int))) return 1;
  clk.mark("operand buffer allocated");
  if (stage_operand(snp_matrix, in_dev, row_bytes, is_plink, g, (uint8_t *)d_X.p, (int *)d_flag.p, bounce, s, 0, post ? k : 0)) return 1;   // GRM / LD: padding bits are no data
  clk.mark("operand staged (upload + k_xstage)");
  bool f4 = false;
  if (pick_engine((const int *)d_flag.p, k, s, f4)) return 1;

  // ---- the route, decided once the engine is known: the result on the device (out_dev), or a host result through ONE copy of an n x n device buffer,
  // through the slab pipeline into that buffer, or through the pipeline's ring of column slabs with no such buffer at all.
  // GRM / LD: the element-wise map is fused into the crossproduct epilogue (whole matrix; MXA_XPROD_FUSED_POST=0 keeps the three extra passes over the result).
  // (rows >= kXFusedMaxRows: the three-pass post-processing runs)
  const int post_kind = post && fused_on && whole && rows < kXFusedMaxRows ? post : kPostNone;
  const bool slabs = pipelined && (!post || post_kind);   // unfused post-processing needs the whole matrix on the device: one copy, even where the ring would go
  // the ring where the call is bound by the download anyway -- the ring computes every off-diagonal tile twice.  Estimates: triangular arithmetic at the
  // measured tile rate against the download at ~55 GB/s of four copiers.  MXA_XPROD_HOST_RING: 0 never, 1 by this estimate (default), 2 always (tests).
  bool ring = false;
  if (slabs) {
    const char *e_ring = getenv("MXA_XPROD_HOST_RING");
    const int ring_mode = e_ring ? atoi(e_ring) : 1;
    const double nbt = (double)g.nb, tri_ms = (double)g.nslabs * tile_stage_ms(f4) * nbt * (nbt + 1.0) / 2.0 / 256.0, copy_ms = (double)abytes / 55e9 * 1e3;
    ring = ring_mode >= 2 || (ring_mode == 1 && abytes >= ((size_t)4 << 30) && 2.0 * tri_ms <= 1.15 * copy_ms);
    if (!ring && ring_mode >= 1) {   // a result that does not fit the free device memory can only leave through the ring
      size_t fb = 0, tb = 0;
      if (hipMemGetInfo(&fb, &tb) == hipSuccess && abytes + ((size_t)1 << 30) > fb) ring = true;
    }
  }
  double *d_ans = out_dev ? ans : nullptr;
  if (!out_dev && !ring) {
    // checked against the free memory first, so that what does not fit is reported like the reference's pre-flight (cuda_utils.cu:162-185) instead of
    // as a raw hipMalloc failure
    size_t fb = 0, tb = 0;
    if (hipMemGetInfo(&fb, &tb) == hipSuccess && abytes > fb) {
      set_error(12, "Not enough device memory available. Required %zu GB, free %zu GB, total on device %zu GB", abytes >> 30, fb >> 30, tb >> 30);
      return 1;
    }
    (void)hipGetLastError();
    if (d_out.alloc(abytes)) return 1;
    d_ans = (double *)d_out.p;
    if (upper_only) MXA_HIP(hipMemsetAsync(d_ans, 0, abytes, s));   // the untouched part travels back as zeros
    clk.mark("device result buffer allocated");
    prefault.start(ans, abytes);
  }
  const double *d_f = freq;
  if (post && freq && ptr_location(freq, nullptr) != 1) {
    const long flen = post == kPostGrm ? k : rows;
    if (f_tmp.alloc(sizeof(double) * flen)) return 1;
    MXA_HIP(hipMemcpyAsync(f_tmp.p, freq, sizeof(double) * flen, hipMemcpyHostToDevice, s));
    d_f = (const double *)f_tmp.p;
  }
  XPost xp;
  XBuf stats[3];
  if (post_kind && fused_post_stats(g, (const uint8_t *)d_X.p, k, post, do_scale, d_f, stats, s, xp)) return 1;
  if (slabs) {
    const int rc = crossprod_slabs(g, (const uint8_t *)d_X.p, d_ans, ans, s, f4, post_kind, xp, ring, prefault);
    clk.mark(ring ? "slabs computed and copied out (ring)" : "tiles computed, slabs copied out");
    d_out.release(); d_X.release();
    clk.mark("device buffers released");
    return rc;
  }
  if (crossprod_device(g, (const uint8_t *)d_X.p, d_ans, s, c_begin, c_end, upper_only, ld, f4, post_kind, xp)) return 1;
  if (post && !post_kind && postprocess_device(d_ans, rows, k, post, do_scale, d_f, s)) return 1;
  clk.mark("tile list built, product enqueued");
  if (!out_dev) MXA_HIP(hipMemcpyAsync(ans, d_ans, abytes, hipMemcpyDeviceToHost, s));
  MXA_HIP(hipStreamSynchronize(s));
  clk.mark("product (and download) finished");
  return 0;
}

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
// A third result of the general window, set_pairs(): the pairs above a cutoff as CSR (mxa_ld_window_pairs*).  `out` is then the caller's rowptr, and a host
// result leaves from one device buffer d_out = rowptr (snps + 1 longs), val (capacity doubles), col (capacity ints); finish_pairs() instead of finish().
struct LdWindow {
  const char *who;
  const unsigned char *plink;
  long snps, indiv, window;
  const int *last;             // the caller's, host or device; nullptr: the fixed window
  double *out;
  long ldb;
  bool scores;
  int flag;                    // kind (band, rows, pairs) / adjust (scores)
  bool pairs = false, fill = false;   // the CSR result; fill: col / val are written (else the count-only call)
  int *col = nullptr;
  double *val = nullptr;
  long capacity = 0;           // entries of col / val (0 on a count-only call)
  bool apply = false;          // the window applied to a matrix (mxa_ld_window_apply*): out = Y, ldb = ldy, result = snps x ncols
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
      : who(who_), plink(plink_), snps(snps_), indiv(indiv_), window(window_), last(last_), out(out_), ldb(ldb_), scores(scores_), flag(flag_), g(indiv_, snps_) {}
  const uint8_t *X() const { return (const uint8_t *)d_X.p; }
  bool general() const { return last != nullptr; }
  // the epilogue kind of the crossproduct kernels and what they take for `c0`
  int post_kind() const { return scores ? kPostLdScores : kPostLdBand; }
  long post_c0() const { return general() ? (long)ndiag : window; }
  void set_post(XPost &xp) const { xp.do_scale = flag; xp.last = (const int *)d_last.p; xp.rowptr = (const long *)d_rowptr.p; }
  std::vector<int4> tiles() const { return window_tiles(jmax); }
  void set_apply(int ncols_) { apply = true; ncols = ncols_; }
  void set_pairs(int *col_, double *val_, long capacity_) { pairs = true; fill = col_ != nullptr; col = col_; val = val_; capacity = fill ? capacity_ : 0; }
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
    if (flag != 0 && flag != 1) { set_error(1, "%s: %s must be 0 or 1", who, scores ? "adjust" : "kind"); return 1; }
    if (!general() && !scores && ldb < window + 1) { set_error(1, "%s: need ldb >= window + 1 (ldb %ld, window %ld)", who, ldb, window); return 1; }
    if (scores && flag && indiv < 3) { set_error(1, adj_msg, who); return 1; }
    if (max_indiv && indiv > max_indiv) { set_error(1, "%s: at most %ld individuals per call (4 indiv^2 must stay below 2^53)", who, max_indiv); return 1; }
    if (snps >= kXFusedMaxRows) { set_error(1, snps_msg, who, kXFusedMaxRows - 1); return 1; }
    if (select_device() < 0) return 1;
    std::vector<long> h_rowptr;
    std::vector<int> h_last;
    if (plan(h_rowptr, h_last)) return 1;
    row_bytes = (indiv + 3) / 4;
    in_dev = ptr_location(plink, nullptr) == 1;
    out_dev = ptr_location(out, nullptr) == 1;
    if (pairs && fill && ((ptr_location(col, nullptr) == 1) != out_dev || (val && (ptr_location(val, nullptr) == 1) != out_dev))) {   // val == nullptr: the library's own "no val" fill
      set_error(1, "%s: rowptr, col and val must be all host or all device pointers", who);
      return 1;
    }
    // a host band leaves from a compact device copy (leading dimension window + 1); the scores' partial buffer holds 2 (ndiag + 1) slots per SNP
    plane_bytes = (size_t)g.rows_pad() * g.pitch();
    obytes = sizeof(double) * (scores ? (size_t)snps : general() ? (size_t)h_rowptr.back() : (size_t)(window + 1) * (size_t)snps);
    if (pairs) obytes = sizeof(long) * ((size_t)snps + 1) + (sizeof(double) + sizeof(int)) * (size_t)capacity;
    if (apply) obytes = sizeof(double) * (size_t)snps * (size_t)ncols;   // a host Y leaves from a compact device copy (leading dimension snps)
    const size_t pbytes = scores ? sizeof(double) * ld_score_slot(2, 0, ndiag, g.rows_pad()) : 0;
    const size_t wbytes = sizeof(int) * (size_t)g.nb + (general() ? sizeof(int) * (size_t)snps + sizeof(long) * ((size_t)snps + 1) : 0);   // jmax, last, rowptr
    size_t free_b = 0, total_b = 0;
    MXA_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t need = planes * plane_bytes + pbytes + wbytes + extra_bytes() + (out_dev ? 0 : obytes) + (in_dev ? 0 : std::min<size_t>((size_t)snps * row_bytes, (size_t)256 << 20));
    if (need > free_b) { set_error(12, "%s: not enough device memory: required %zu GB, free %zu GB", who, need >> 30, free_b >> 30); return 1; }
    if (st.create(hipStreamDefault)) return 1;   // blocking: ordered against the caller's default-stream work
    s = st.s;
    if (d_X.alloc(planes * plane_bytes) || d_flag.alloc(sizeof(int)) || (!out_dev && d_out.alloc(obytes)) || (scores && d_P.alloc(pbytes))) return 1;
    // the plan's arrays: synchronous copies (the host vectors end with this function)
    if (scores) {
      if (d_jmax.alloc(sizeof(int) * (size_t)g.nb)) return 1;
      MXA_HIP(hipMemcpy(d_jmax.p, jmax.data(), sizeof(int) * (size_t)g.nb, hipMemcpyHostToDevice));
    }
    if (general()) {
      const bool rows = !scores && !pairs && !apply;   // the ragged rows' starts
      if (d_last.alloc(sizeof(int) * (size_t)snps) || (rows && d_rowptr.alloc(sizeof(long) * ((size_t)snps + 1)))) return 1;
      MXA_HIP(hipMemcpy(d_last.p, h_last.data(), sizeof(int) * (size_t)snps, hipMemcpyHostToDevice));
      if (rows) MXA_HIP(hipMemcpy(d_rowptr.p, h_rowptr.data(), sizeof(long) * ((size_t)snps + 1), hipMemcpyHostToDevice));
    }
    d_res = out_dev ? out : (double *)d_out.p;
    ld_res = out_dev ? ldb : window + 1;
    d_dst = scores ? (double *)d_P.p : d_res;
    ld_dst = scores ? g.rows_pad() : ld_res;
    return e0.create() || e1.create();
  }
  int start() { MXA_HIP(hipEventRecord(e0.e, s)); return 0; }
  int finish() {
    if (scores) hipLaunchKernelGGL(k_ld_score_finish, dim3((unsigned)((snps + 255) / 256)), dim3(256), 0, s, (const double *)d_P.p, snps, g.rows_pad(), (const int *)d_jmax.p, ndiag, d_res);
    else if (!general() && window > 0) hipLaunchKernelGGL(k_ld_band_tail, dim3((unsigned)window), dim3(256), 0, s, d_res, ld_res, snps, window);
    MXA_HIP(hipGetLastError());
    MXA_HIP(hipEventRecord(e1.e, s));
    if (!out_dev && ld_window_download(d_res, obytes, snps, window, out, ldb, scores || general(), s)) return 1;
    MXA_HIP(hipStreamSynchronize(s));   // lifetime of the route's tile lists, statistics and scratch
    MXA_HIP(profile_launch(e0, e1));
    return 0;
  }
  // the applied window: Y is complete on the device (d_res, leading dimension out_dev ? ldb : snps); a host Y takes its snps rows of every column
  int finish_apply() {
    MXA_HIP(hipEventRecord(e1.e, s));
    if (!out_dev) MXA_HIP(hipMemcpy2DAsync(out, sizeof(double) * (size_t)ldb, d_res, sizeof(double) * (size_t)snps, sizeof(double) * (size_t)snps, (size_t)ncols, hipMemcpyDeviceToHost, s));
    MXA_HIP(hipStreamSynchronize(s));   // lifetime of the route's tile lists, statistics, scratch and partials
    MXA_HIP(profile_launch(e0, e1));
    return 0;
  }
  // the CSR result: the total (d_total, the running base after the last group) is read once; a host result is rowptr and the first min(total, capacity)
  // entries of col / val.  total > capacity: error 25, rowptr and *total valid.
  int finish_pairs(const long *d_total, long *total) {
    MXA_HIP(hipEventRecord(e1.e, s));
    long h_total = 0;
    MXA_HIP(hipMemcpyAsync(&h_total, d_total, sizeof(long), hipMemcpyDeviceToHost, s));
    if (!out_dev) MXA_HIP(hipMemcpyAsync(out, d_pairs_rowptr(), sizeof(long) * ((size_t)snps + 1), hipMemcpyDeviceToHost, s));
    MXA_HIP(hipStreamSynchronize(s));   // lifetime of the route's tile lists, statistics and scratch
    const size_t filled = (size_t)std::min(h_total, capacity);
    if (!out_dev && filled) {
      MXA_HIP(hipMemcpyAsync(val, d_pairs_val(), sizeof(double) * filled, hipMemcpyDeviceToHost, s));
      MXA_HIP(hipMemcpyAsync(col, d_pairs_col(), sizeof(int) * filled, hipMemcpyDeviceToHost, s));
      MXA_HIP(hipStreamSynchronize(s));
    }
    MXA_HIP(profile_launch(e0, e1));
    *total = h_total;
    if (fill && h_total > capacity) { set_error(25, "%s: %ld pairs pass the cutoff, capacity is %ld", who, h_total, capacity); return 1; }
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
constexpr long kPwMaxIndiv = 47453132L;   // 4 indiv^2 < 2^53
constexpr int kPwPairs = 6;
// the operand planes (A side from the I rows, B side from the J rows) of the six products, in slot order: N, Sxy, Sx, Sy, A_i.M_j, M_i.A_j
__host__ __device__ constexpr int pw_plane_a(int k) { return k == 0 ? 1 : k == 1 ? 0 : k == 2 ? 0 : k == 3 ? 1 : k == 4 ? 2 : 1; }
__host__ __device__ constexpr int pw_plane_b(int k) { return k == 0 ? 1 : k == 1 ? 0 : k == 2 ? 1 : k == 3 ? 0 : k == 4 ? 1 : 2; }

__device__ __forceinline__ double pw_r(double N, double Sxy, double Sx, double Sy, double Ax, double Ay) {
  const double Sxx = Sx + 2.0 * Ax, Syy = Sy + 2.0 * Ay;
  const double num = N * Sxy - Sx * Sy, dx = N * Sxx - Sx * Sx, dy = N * Syy - Sy * Sy;   // exact integers
  return __ddiv_rn(num, __dsqrt_rn(__dmul_rn(dx, dy)));                                    // dx dy = 0 (no shared individuals, or a SNP constant on them): 0 / 0 = NaN
}
// !SCORES: the stored entry r (ld_window_store squares it for kind 1); SCORES: the score term t(r) with the pair's own N, every operation rounded on its own
template <bool SCORES>
__device__ __forceinline__ double pw_value(double N, double Sxy, double Sx, double Sy, double Ax, double Ay, bool adjust) {
  const double r = pw_r(N, Sxy, Sx, Sy, Ax, Ay);
  if constexpr (!SCORES) return r;
  const double r2 = __dmul_rn(r, r);
  return adjust ? __dsub_rn(r2, __ddiv_rn(__dsub_rn(1.0, r2), __dsub_rn(N, 2.0))) : r2;
}

// One workgroup per band tile, the lane <-> element map of the crossproduct epilogue: thread t reads quad q of its sub-block (a, b) at slot + ((4 a + b) 4 + q) 1024 + 4 t,
// where xprod_store_counts wrote it.  DENSE: the six counts of the tile's slots t.w .. t.w + 5.  !DENSE (no missing code in the whole matrix): slot t.w holds
// Sxy only; M is all ones, so N = indiv and the other four are the per-SNP sums sz = sum z, sa = sum a (k_pw_rowsums) -- the same integers, hence the same bits.
// Win: the window object, by value (LdFixedWindow: the band or its scores; LdVarWindow: ragged rows or their scores).
template <bool SCORES, bool DENSE, typename Win>
__global__ void __launch_bounds__(256) k_ld_pw_combine(const int *__restrict__ scratch, const int4 *__restrict__ btiles, const int *__restrict__ sz, const int *__restrict__ sa,
                                                       long n, double indiv, double *__restrict__ out, long ld, Win win, int flag) {
  __shared__ __attribute__((aligned(16))) char smem[kXScratchBytes + (SCORES ? 2 * 4 * 2 * 4 * 32 * 8 : 0)];
  const int4 t = btiles[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wi = wave >> 1, wj = wave & 1;
  const long i0 = (long)t.x * kXT, j0 = (long)t.y * kXT;
  const int4 *base = reinterpret_cast<const int4 *>(scratch + (size_t)t.w * kPwSlotInts) + threadIdx.x;
  constexpr size_t kSlotQuads = kPwSlotInts / 4;
  const int col = lane & 31, rq = 4 * (lane >> 5);
  const bool adjust = flag != 0;
  int cnt[DENSE ? kPwPairs : 1][16];                         // the counts of the current sub-block, in accumulator register order
  long gi_base = 0, gj = 0;
  auto prep = [&](int a, int b) {
    gi_base = i0 + wi * 128 + a * 32; gj = j0 + wj * 128 + b * 32 + col;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int4 *p = base + ((a * 4 + b) * 4 + q) * 256;
#pragma unroll
      for (int k = 0; k < (DENSE ? kPwPairs : 1); k++) {
        const int4 w = p[(size_t)k * kSlotQuads];
        cnt[k][4 * q] = w.x; cnt[k][4 * q + 1] = w.y; cnt[k][4 * q + 2] = w.z; cnt[k][4 * q + 3] = w.w;
      }
    }
  };
  auto val = [&](int, int, int r) -> double {
    if constexpr (DENSE) return pw_value<SCORES>((double)cnt[0][r], (double)cnt[1][r], (double)cnt[2][r], (double)cnt[3][r], (double)cnt[4][r], (double)cnt[5][r], adjust);
    else {
      const long gi = gi_base + (r & 3) + 8 * (r >> 2) + rq;     // row of accumulator register r
      return pw_value<SCORES>(indiv, (double)cnt[0][r], (double)sz[gi], (double)sz[gj], (double)sa[gi], (double)sa[gj], adjust);
    }
  };
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
  LdGroups(const LdWindow &c, size_t cap, int pairs, size_t tile_extra = 0) : row0{0} {
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
}  // namespace

// the pairwise route: the three planes staged, per group of tile rows the count products and their combine
int ld_pairwise_any(const char *who, const unsigned char *plink, long snps, long indiv, long window, const int *last, double *out, long ldb, bool scores, int flag) {
  // the scratch of a group: `pairs` slots of 256 KiB per band tile, tile rows per group so that it stays under the cap (one tile row at least); read per call
  const size_t cap = ld_scratch_cap();
  const size_t slot_bytes = kPwSlotBytes;
  LdWindow c(who, plink, snps, indiv, window, last, out, ldb, scores, flag);
  // (the scratch is counted at its cap -- or at the one tile row of six products it cannot go below -- unless the whole window needs less)
  if (c.begin(3, [&] { return std::min(std::max(cap, c.row_tiles_max * kPwPairs * slot_bytes), c.ntiles * kPwPairs * slot_bytes); }, nullptr, kPwMaxIndiv,
              "%s: the adjusted estimator r^2 - (1 - r^2) / (N - 2) needs indiv >= 3", "%s: at most %ld SNPs per call")) return 1;
  const XGeom &g = c.g;
  hipStream_t s = c.s;
  XBuf d_scr, d_bt;
  LdPairwiseOperand op;
  if (op.stage(c, plink)) return 1;
  const bool f4 = op.f4, dense = op.dense;
  const int pairs = op.pairs;
  int *d_sz = op.d_sz, *d_sa = op.d_sa;
  LdGroups gr(c, cap, pairs);
  const int ngroups = gr.n;
  const std::vector<int> &group_row0 = gr.row0;
  const std::vector<size_t> &band_first = gr.band_first;
  XTiles t;
  if (upload_tiles(std::move(gr.prod), s, t)) return 1;
  if (d_bt.alloc(gr.band.size() * sizeof(int4)) || d_scr.alloc(gr.tiles_max * (size_t)pairs * slot_bytes)) return 1;
  MXA_HIP(hipMemcpyAsync(d_bt.p, gr.band.data(), gr.band.size() * sizeof(int4), hipMemcpyHostToDevice, s));
  if (c.start()) return 1;
  const XPost none{};
  for (int q = 0; q < ngroups; q++) {
    // the products of the group into the scratch, then its combine, one behind the other on the call's stream (the next group reuses the scratch)
    if (t.launch(q, g, f4, s, c.X(), (double *)d_scr.p, 0, 0, nullptr, kPostCounts, none)) return 1;
    const dim3 grid((unsigned)(band_first[(size_t)q + 1] - band_first[(size_t)q]));
    const int4 *bt = (const int4 *)d_bt.p + band_first[(size_t)q];
    // the instantiation for (scores, dense, window object)
    auto combine = [&](auto win) {
      using Win = decltype(win);
      auto go = [&](auto k) { hipLaunchKernelGGL(k, grid, dim3(256), 0, s, (const int *)d_scr.p, bt, (const int *)d_sz, (const int *)d_sa, snps, (double)indiv, c.d_dst, c.ld_dst, win, flag); };
      if (scores) { if (dense) go(k_ld_pw_combine<true, true, Win>); else go(k_ld_pw_combine<true, false, Win>); }
      else { if (dense) go(k_ld_pw_combine<false, true, Win>); else go(k_ld_pw_combine<false, false, Win>); }
    };
    if (c.general()) combine(LdVarWindow{(const int *)c.d_last.p, (const long *)c.d_rowptr.p, c.ndiag});
    else combine(LdFixedWindow{window});
    MXA_HIP(hipGetLastError());
  }
  if (c.finish()) return 1;
  debug_info("%s: %d group(s) of up to %d tile rows, %d product(s) per band tile (%s), %s engine", who, ngroups, group_row0[1], pairs, dense ? "six counts" : "no missing code: per-SNP sums",
             f4 ? "FP4" : "int8");
  return 0;
}

// ---- pairs above a cutoff as CSR (mxa_ld_window_pairs, mxa_ld_window_pairs_pairwise): the candidates i < j <= last[i] whose q = fl(r r) >= min_r2, compacted
// on the device.  Both routes run the window's tile products once into the count scratch (kPostCounts; the plain route one slot per window tile), in the
// groups of LdGroups; per group k_ld_select counts (WRITE = false), the scan kernels turn the counts into positions, and k_ld_select runs again and writes
// (WRITE = true), recomputing its masks from the scratch, which is still in place.  Every position is a sum of counts in a fixed order: no atomics.
// The providers: r of one element from the counts of its sub-block (cnt[slot][register], the lane <-> element map of k_ld_pw_combine), bit for bit what the
// rows entries store at kind 0 -- the plain map of xprod_store_window's fin, or pw_r as k_ld_pw_combine calls it.
struct LdPairsPlain {
  static constexpr int kSlots = 1;
  const double *__restrict__ u, *__restrict__ w;
  double a;
  __device__ __forceinline__ double r(const int (&cnt)[kSlots][16], int reg, long gi, long gj) const {
    return ld_scale_map(ld_center_map((double)cnt[0][reg], u[gj], u[gi], a), w[gj], w[gi]);
  }
};
struct LdPairsCounts {
  static constexpr int kSlots = kPwPairs;
  __device__ __forceinline__ double r(const int (&cnt)[kSlots][16], int reg, long, long) const {
    return pw_r((double)cnt[0][reg], (double)cnt[1][reg], (double)cnt[2][reg], (double)cnt[3][reg], (double)cnt[4][reg], (double)cnt[5][reg]);
  }
};
struct LdPairsSums {
  static constexpr int kSlots = 1;
  const int *__restrict__ sz, *__restrict__ sa;
  double indiv;
  __device__ __forceinline__ double r(const int (&cnt)[kSlots][16], int reg, long gi, long gj) const {
    return pw_r(indiv, (double)cnt[0][reg], (double)sz[gi], (double)sz[gj], (double)sa[gi], (double)sa[gj]);
  }
};
// The one decision of both passes: q = fl(r r), kept iff q >= min_r2 (a NaN r: the comparison is false).  Nothing here can be contracted.
__device__ __forceinline__ bool ld_pair_keep(double r, double min_r2, double &q) {
  q = __dmul_rn(r, r);
  return q >= min_r2;
}

// One workgroup per window tile.  Element (gi, gj) of the tile is held by the lane the crossproduct epilogue gives it: lane & 31 runs along gj, the two 32-lane
// halves of a wave hold rows 4 apart, so a ballot is two 32-bit words of the table mask[row][word], word = the row's 32-column sub-block, ascending in gj.
// Count pass: cnt[tile][row] = the row's popcount.  Write pass: cnt holds rel[tile][row], the row's kept pairs in the tiles to the left (k_ld_pairs_rowscan);
// position = rowptr[gi] + rel + popcounts of the row's lower words + of its own word below the lane; a position >= capacity is dropped.
// val == nullptr (the selection entries, which need the graph alone): the write pass still rebuilds its masks from the counts in the first loop, as ever; its
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
  const int4 *slot = reinterpret_cast<const int4 *>(scratch + (size_t)t.w * kPwSlotInts) + tid;
  constexpr size_t kSlotQuads = kPwSlotInts / 4;
  const int c = lane & 31, hh = lane >> 5;
  int counts[Prov::kSlots][16];                              // the counts of the current sub-block, in accumulator register order
  auto load = [&](int a, int b) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int4 *p = slot + ((a * 4 + b) * 4 + q) * 256;
#pragma unroll
      for (int k = 0; k < Prov::kSlots; k++) {
        const int4 w = p[(size_t)k * kSlotQuads];
        counts[k][4 * q] = w.x; counts[k][4 * q + 1] = w.y; counts[k][4 * q + 2] = w.z; counts[k][4 * q + 3] = w.w;
      }
    }
  };
#pragma unroll
  for (int k = 0; k < 8; k++) mask[tid][k] = 0u;             // sub-blocks skipped below keep no pair
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const long gi_base = i0 + wi * 128 + a * 32, gj_base = j0 + wj * 128 + b * 32;
      if (gj_base + 31 <= gi_base || win.beyond(gi_base, gj_base, n)) continue;   // wave-uniform: no element above the diagonal, or none within the window
      load(a, b);
      const long gj = gj_base + c;
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const int row = (reg & 3) + 8 * (reg >> 2) + 4 * hh;
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
        if (want_val) load(a, b);
        const long gj = gj_base + c;
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
          const int row = wi * 128 + a * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * hh, word = wj * 4 + b;
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
// with col alone (ld_prune_window); the public entries pass false and reject a lone NULL as ever.
static int ld_pairs_any(const char *who, const unsigned char *plink, long snps, long indiv, const int *last, double min_r2, int kind, long *rowptr, int *col, double *val,
                        long capacity, long *total, bool pairwise, bool is_plink, const double *freq, bool no_val = false) {
  if (!last || !rowptr || !total) { set_error(1, "%s: bad arguments", who); return 1; }
  if (!no_val && (col == nullptr) != (val == nullptr)) { set_error(1, "%s: col and val must both be given (the filling call) or both be NULL (the count-only call)", who); return 1; }
  if (col && capacity < 0) { set_error(1, "%s: capacity must not be negative (%ld)", who, capacity); return 1; }
  if (!(min_r2 >= 0.0) || min_r2 > DBL_MAX) { set_error(1, "%s: min_r2 must be finite and not negative", who); return 1; }
  const size_t cap = ld_scratch_cap();
  LdWindow c(who, plink, snps, indiv, 0, last, reinterpret_cast<double *>(rowptr), 0, false, kind);
  c.set_pairs(col, val, capacity);
  const int pairs_max = pairwise ? kPwPairs : 1;
  // the scratch as ld_pairwise_any counts it, the per-(tile, row) counters of a group (1 KiB per window tile), and per tile row tfirst and the row sums
  auto extra = [&] {
    const size_t scr = std::min(std::max(cap, c.row_tiles_max * pairs_max * kPwSlotBytes), c.ntiles * pairs_max * kPwSlotBytes);
    return scr + std::min(c.ntiles, std::max(cap / kPwSlotBytes, c.row_tiles_max)) * kXT * sizeof(int) + sizeof(long) * (2 * (size_t)c.g.nb + 2);
  };
  if (c.begin(pairwise ? 3 : 1, extra, pairwise || freq ? nullptr : "%s: allele frequencies are required", pairwise ? kPwMaxIndiv : 0L, "%s",
              pairwise ? "%s: at most %ld SNPs per call" : "%s: at most %ld SNPs per call (the fused statistics)")) return 1;
  const XGeom &g = c.g;
  hipStream_t s = c.s;
  LdPlainOperand plain;
  LdPairwiseOperand pw;
  if (pairwise ? pw.stage(c, plink) : plain.stage(c, plink, is_plink, freq)) return 1;
  const bool f4 = pairwise ? pw.f4 : plain.f4;
  const int pairs = pairwise ? pw.pairs : 1;
  LdGroups gr(c, cap, pairs);
  std::vector<long> tfirst((size_t)g.nb + 1, 0);
  for (int I = 0; I < g.nb; I++) tfirst[(size_t)I + 1] = tfirst[(size_t)I] + (c.jmax[(size_t)I] - I + 1);
  XTiles t;
  XBuf d_scr, d_bt, d_cnt, d_rows;                           // d_rows: tfirst (nb + 1 longs), the groups' row sums (nb), the running base (1)
  if (upload_tiles(std::move(gr.prod), s, t)) return 1;
  if (d_bt.alloc(gr.band.size() * sizeof(int4)) || d_scr.alloc(gr.tiles_max * (size_t)pairs * kPwSlotBytes) || d_cnt.alloc(gr.tiles_max * kXT * sizeof(int)) ||
      d_rows.alloc(sizeof(long) * (2 * (size_t)g.nb + 2))) return 1;
  long *d_tfirst = (long *)d_rows.p, *d_rowsum = d_tfirst + g.nb + 1, *d_base = d_rowsum + g.nb;
  MXA_HIP(hipMemcpyAsync(d_bt.p, gr.band.data(), gr.band.size() * sizeof(int4), hipMemcpyHostToDevice, s));
  MXA_HIP(hipMemcpyAsync(d_tfirst, tfirst.data(), sizeof(long) * tfirst.size(), hipMemcpyHostToDevice, s));
  MXA_HIP(hipMemsetAsync(d_base, 0, sizeof(long), s));
  if (c.start()) return 1;
  const XPost none{};
  const LdVarWindow win{(const int *)c.d_last.p, nullptr, c.ndiag};
  long *d_rowptr = c.d_pairs_rowptr();
  for (int q = 0; q < gr.n; q++) {
    // the group's products into the scratch; count; scan (the running base crosses the groups on the device: the host does not wait); write
    if (t.launch(q, g, f4, s, c.X(), (double *)d_scr.p, 0, 0, nullptr, kPostCounts, none)) return 1;
    const dim3 grid((unsigned)(gr.band_first[(size_t)q + 1] - gr.band_first[(size_t)q]));
    const int4 *bt = (const int4 *)d_bt.p + gr.band_first[(size_t)q];
    const int i_lo = gr.row0[(size_t)q], nrows = gr.row0[(size_t)q + 1] - i_lo;
    auto select = [&](auto write, auto prov) {
      hipLaunchKernelGGL((k_ld_select<decltype(write)::value, decltype(prov), LdVarWindow>), grid, dim3(256), 0, s, (const int *)d_scr.p, bt, snps, prov, win, min_r2, kind,
                         (int *)d_cnt.p, (const long *)d_rowptr, c.d_pairs_col(), c.d_pairs_val(), c.capacity);
    };
    auto pass = [&](auto write) {
      if (!pairwise) select(write, LdPairsPlain{plain.xp.u, plain.xp.w, plain.xp.a});
      else if (pw.dense) select(write, LdPairsCounts{});
      else select(write, LdPairsSums{pw.d_sz, pw.d_sa, (double)indiv});
    };
    pass(std::false_type());
    hipLaunchKernelGGL(k_ld_pairs_rowscan, dim3((unsigned)nrows), dim3(256), 0, s, (int *)d_cnt.p, (const long *)d_tfirst, i_lo, snps, d_rowptr, d_rowsum);
    hipLaunchKernelGGL(k_ld_pairs_groupscan, dim3(1), dim3(1024), 0, s, d_rowsum, nrows, d_base);
    hipLaunchKernelGGL(k_ld_pairs_rowptr, dim3((unsigned)nrows), dim3(256), 0, s, d_rowptr, (const long *)d_rowsum, i_lo, snps, (const long *)d_base, q == gr.n - 1 ? 1 : 0);
    if (c.fill) pass(std::true_type());
    MXA_HIP(hipGetLastError());
  }
  if (c.finish_pairs(d_base, total)) return 1;
  debug_info("%s: %d group(s), %d product(s) per window tile, %s engine, %ld pairs", who, gr.n, pairs, f4 ? "FP4" : "int8", *total);
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
  if constexpr (__is_same(Prov, LdPairsPlain)) {
    const double p = q * inv_adj;
    return r2 - p;
  } else {
    double N;
    if constexpr (__is_same(Prov, LdPairsCounts)) N = (double)cnt[0][reg]; else N = prov.indiv;
    const double p = q / (N - 2.0);
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
  if constexpr (__is_same(Prov, LdPairsPlain)) inv_adj = term == 2 ? 1.0 / (prov.a * 0.25 - 2.0) : 0.0;   // prov.a = 4 indiv
  for (int e = tid; e < 2 * kXT * NC; e += 256) {           // e = (side NC + k) 256 + row: the threads run along the rows of a column of X
    const int row = e & (kXT - 1), k = (e >> 8) % NC, side = e / (kXT * NC);
    const long g = (side ? j0 : i0) + row;
    xs[(side * kXT + row) * NC + k] = g < n && c0 + k < ncols ? X[(size_t)g + (size_t)(c0 + k) * (size_t)ldx] : 0.0;
  }
  __syncthreads();
  const int4 *slot = reinterpret_cast<const int4 *>(scratch + (size_t)t.w * kPwSlotInts) + tid;
  constexpr size_t kSlotQuads = kPwSlotInts / 4;
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
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int4 *p = slot + ((a * 4 + b) * 4 + q) * 256;
#pragma unroll
        for (int k = 0; k < Prov::kSlots; k++) {
          const int4 w = p[(size_t)k * kSlotQuads];
          counts[k][4 * q] = w.x; counts[k][4 * q + 1] = w.y; counts[k][4 * q + 2] = w.z; counts[k][4 * q + 3] = w.w;
        }
      }
      const long gj = gj_base + c;
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const int row = (reg & 3) + 8 * (reg >> 2) + 4 * hh;
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
  const int pairs_max = pairwise ? kPwPairs : 1;
  const size_t part_bytes = sizeof(double) * 2 * kXT * (size_t)n;   // the partials of a window tile: they share the cap with its count slots
  bool x_dev = false;
  // the scratch and the partials as ld_pairwise_any counts the scratch, the device copy of a host X, the window tiles' list and the plan's arrays
  auto extra = [&] {
    x_dev = ptr_location(X, nullptr) == 1;
    const size_t tile_bytes = pairs_max * kPwSlotBytes + part_bytes;
    return std::min(std::max(cap, c.row_tiles_max * tile_bytes), c.ntiles * tile_bytes) + (x_dev ? 0 : sizeof(double) * (size_t)snps * (size_t)n) +
           c.ntiles * sizeof(int4) + sizeof(long) * ((size_t)c.g.nb + 1) + 2 * sizeof(int) * (size_t)c.g.nb;
  };
  if (c.begin(pairwise ? 3 : 1, extra, pairwise || freq ? nullptr : "%s: allele frequencies are required", pairwise ? kPwMaxIndiv : 0L, "%s",
              pairwise ? "%s: at most %ld SNPs per call" : "%s: at most %ld SNPs per call (the fused statistics)")) return 1;
  const XGeom &g = c.g;
  hipStream_t s = c.s;
  LdPlainOperand plain;
  LdPairwiseOperand pw;
  if (pairwise ? pw.stage(c, plink) : plain.stage(c, plink, is_plink, freq)) return 1;
  const bool f4 = pairwise ? pw.f4 : plain.f4;
  const int pairs = pairwise ? pw.pairs : 1;
  LdGroups gr(c, cap, pairs, part_bytes);
  // the plan's arrays on the device: tfirst (nb + 1 longs), then jmax and imin (nb ints each)
  std::vector<long> tfirst((size_t)g.nb + 1, 0);
  std::vector<int> imin((size_t)g.nb, 0);
  for (int I = 0; I < g.nb; I++) tfirst[(size_t)I + 1] = tfirst[(size_t)I] + (c.jmax[(size_t)I] - I + 1);
  for (int B = 0, I = 0; B < g.nb; B++) { while (c.jmax[(size_t)I] < B) I++; imin[(size_t)B] = I; }   // jmax[B] >= B ends the search
  XTiles t;
  XBuf d_scr, d_bt, d_part, d_plan, d_xm;
  if (upload_tiles(std::move(gr.prod), s, t)) return 1;
  if (d_bt.alloc(gr.band.size() * sizeof(int4)) || d_scr.alloc(gr.tiles_max * (size_t)pairs * kPwSlotBytes) || d_part.alloc(gr.tiles_max * part_bytes) ||
      d_plan.alloc(sizeof(long) * ((size_t)g.nb + 1) + 2 * sizeof(int) * (size_t)g.nb) || (!x_dev && d_xm.alloc(sizeof(double) * (size_t)snps * (size_t)n))) return 1;
  long *d_tfirst = (long *)d_plan.p;
  int *d_jmax = (int *)(d_tfirst + g.nb + 1), *d_imin = d_jmax + g.nb;
  MXA_HIP(hipMemcpyAsync(d_bt.p, gr.band.data(), gr.band.size() * sizeof(int4), hipMemcpyHostToDevice, s));
  MXA_HIP(hipMemcpyAsync(d_tfirst, tfirst.data(), sizeof(long) * tfirst.size(), hipMemcpyHostToDevice, s));
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
  const XPost none{};
  const LdVarWindow win{(const int *)c.d_last.p, nullptr, c.ndiag};
  const unsigned chunks = (unsigned)((n + kLdApplyNC - 1) / kLdApplyNC);
  static unsigned long long lds_mask[3] = {0, 0, 0};
  for (int q = 0; q < gr.n; q++) {
    // the group's products into the scratch, its tiles' partials, and the partials into Y (the next group reuses the scratch and the partials)
    if (t.launch(q, g, f4, s, c.X(), (double *)d_scr.p, 0, 0, nullptr, kPostCounts, none)) return 1;
    const dim3 grid((unsigned)(gr.band_first[(size_t)q + 1] - gr.band_first[(size_t)q]), chunks);
    const int4 *bt = (const int4 *)d_bt.p + gr.band_first[(size_t)q];
    auto tile = [&](auto prov, int which) {
      constexpr auto K = &k_ld_apply_tile<decltype(prov), LdVarWindow>;
      if (ensure_dyn_lds(reinterpret_cast<const void *>(K), kLdApplyLds, &lds_mask[which])) return 1;
      hipLaunchKernelGGL(K, grid, dim3(256), kLdApplyLds, s, (const int *)d_scr.p, bt, snps, prov, win, term, d_x, ld_x, (int)n, (double *)d_part.p);
      return 0;
    };
    if (!pairwise ? tile(LdPairsPlain{plain.xp.u, plain.xp.w, plain.xp.a}, 0) : pw.dense ? tile(LdPairsCounts{}, 1) : tile(LdPairsSums{pw.d_sz, pw.d_sa, (double)indiv}, 2)) return 1;
    const int i_lo = gr.row0[(size_t)q], i_hi = gr.row0[(size_t)q + 1];
    const long nrows = std::min(snps, ((long)c.jmax[(size_t)i_hi - 1] + 1) * kXT) - (long)i_lo * kXT;
    // One thread per (row, column) of the group: the limit of a launch is 2^32 threads, not 2^31 workgroups, so this goes in pieces as well (every thread
    // owns its Y[i, c]: no order between the pieces).  No test reaches the second piece: under the default 2 GiB scratch cap a group holds nrows n <= 2^26,
    // and 2^32 (row, column) pairs in one group need more than 100 GB of partial sums.
    launch_in_block_chunks((nrows * n + 255) / 256, [&](unsigned nb, long blk0) {
      hipLaunchKernelGGL(k_ld_apply_finish, dim3(nb), dim3(256), 0, s, (const double *)d_part.p, (int)n, (const long *)d_tfirst, (const int *)d_jmax,
                         (const int *)d_imin, i_lo, i_hi, snps, nrows, d_y, ld_y, blk0);
    });
    MXA_HIP(hipGetLastError());
  }
  if (c.finish_apply()) return 1;
  debug_info("%s: %d group(s), %d product(s) per window tile, %s engine, %ld column(s) in %u chunk(s)", who, gr.n, pairs, f4 ? "FP4" : "int8", n, chunks);
  return 0;
}

// ---- greedy selection on the pairs graph (mxa_ld_prune_csr, mxa_ld_window_prune, mxa_ld_window_prune_pairwise).  G: the strict upper CSR (rowptr, col) read as
// an undirected graph.  a comes before b iff priority[a] < priority[b], or they are equal and a < b (priority == nullptr: a < b).  Result: the greedy walk in
// that order -- keep a SNP iff none of its neighbours is kept --, i.e. the lexicographically first maximal independent set, which is unique: nothing below
// depends on a schedule.  state[v]: 0 undecided, r > 0 kept in round r, kPruneRemoved.  Round r = 1, 2, .. is two launches that end on their own:
//   k_ld_prune_edges     one wave per row i of the upper CSR, lanes over its columns j, reading the states round r - 1 left.  Row i is active iff i is undecided or
//                        was kept in round r - 1:  i kept in r - 1, j undecided: rm[j] = r;  i undecided, j kept (any age): rm[i] = r;  both undecided:
//                        bl[the later one] = r.  rm ("remove") and bl ("blocked") are round stamps: every writer of a round writes the same r, rounds only
//                        grow, so they are never cleared.
//   k_ld_prune_vertices  an undecided v with rm[v] == r is removed; else with bl[v] != r it is kept (state r); else it waits.  One integer atomicAdd per
//                        workgroup of its undecided and of its kept count (integer sums: no order).
// The upper triangle suffices: an edge {i < j} with an undecided endpoint has i undecided (row i is active), or i kept -- then row i was active in the round after
// i was kept and removed every undecided upper neighbour, j among them --, or i removed, and then nothing is to do.  A kept j > i is seen from row i, which is
// active while i is undecided.  v is kept only when all its earlier neighbours are removed and none is kept, which is the walk's decision; v is removed only next
// to a kept SNP, and that SNP comes before v (it was kept with all its earlier neighbours decided).  The first undecided SNP in the order is never blocked, so
// every round decides one: rounds <= snps.
// The host enqueues the rounds in batches (kPruneBatch0 rounds, doubling up to kPruneBatchMax) and reads the batch's undecided counts once; the first zero is
// the round of convergence, so `rounds` does not depend on the batching, and a round behind it returns at its first load (und_prev).
constexpr int kPruneRemoved = -1, kPruneBatch0 = 8, kPruneBatchMax = 128, kPruneNoOwner = 0x7fffffff;
constexpr unsigned long long kPruneNoKey = ~0ull;

// a 64-bit key with key(p) < key(q) iff p < q for all non-NaN doubles; -0.0 and +0.0 share one key
__device__ __forceinline__ unsigned long long prune_key(double p) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(p + 0.0);
  return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}

__global__ void __launch_bounds__(256) k_ld_prune_edges(const long *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ prio, long n, int round,
                                                        const int *__restrict__ state, int *__restrict__ rm, int *__restrict__ bl, const int *__restrict__ und_prev,
                                                        long blk0) {
  if (und_prev && *und_prev == 0) return;                    // converged in an earlier round of this batch
  const long i = (blk0 + blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int lane = threadIdx.x & 63, si = state[i];
  if (si != 0 && (si != round - 1 || round == 1)) return;   // neither undecided nor kept in the previous round (kPruneRemoved is never round - 1)
  const long k1 = rowptr[i + 1];
  const double pi = prio ? prio[i] : 0.0;
  bool remove_i = false, block_i = false;
  for (long k = rowptr[i] + lane; k < k1; k += 64) {
    const int j = col[k], sj = state[j];
    if (si != 0) {
      if (sj == 0) atomicMax(&rm[j], round);
    } else if (sj > 0) remove_i = true;
    else if (sj == 0) {                                      // i < j: i comes first unless j's priority is strictly smaller
      if (prio && prio[j] < pi) block_i = true;
      else atomicMax(&bl[j], round);
    }
  }
  if (remove_i) atomicMax(&rm[i], round);
  if (block_i) atomicMax(&bl[i], round);
}

__global__ void __launch_bounds__(256) k_ld_prune_vertices(long n, int round, int *__restrict__ state, const int *__restrict__ rm, const int *__restrict__ bl,
                                                           int *__restrict__ und, unsigned long long *__restrict__ kept, const int *__restrict__ und_prev) {
  if (und_prev && *und_prev == 0) return;
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  int waits = 0, keeps = 0;
  if (v < n && state[v] == 0) {
    if (rm[v] == round) state[v] = kPruneRemoved;
    else if (bl[v] != round) { state[v] = round; keeps = 1; }
    else waits = 1;
  }
  const int nw = __syncthreads_count(waits), nk = __syncthreads_count(keeps);
  if (threadIdx.x == 0) {
    if (nw) atomicAdd(und, nw);
    if (nk) atomicAdd(kept, (unsigned long long)nk);
  }
}

// the results from the final states: keep, and the start of the owner pass (a kept SNP owns itself)
__global__ void __launch_bounds__(256) k_ld_prune_result(long n, const int *__restrict__ state, unsigned char *__restrict__ keep, int *__restrict__ owner,
                                                         unsigned long long *__restrict__ key) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const bool kept = state[v] > 0;
  keep[v] = kept ? 1 : 0;
  if (owner) owner[v] = kept ? (int)v : kPruneNoOwner;
  if (key) key[v] = kPruneNoKey;
}

// The owner pass, once after convergence, one wave per row over all rows: on every edge with exactly one kept endpoint the dropped endpoint takes the minimum
// over its kept neighbours in the order.  KEY: atomicMin of the neighbours' priority keys; then (!KEY) atomicMin of the index among the neighbours whose key is
// that minimum (prio == nullptr: every neighbour).  The row's own minimum is reduced over the wave first: one atomic per row for it.
template <bool KEY>
__global__ void __launch_bounds__(256) k_ld_prune_owner(const long *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ prio, long n,
                                                        const int *__restrict__ state, unsigned long long *__restrict__ key, int *__restrict__ owner, long blk0) {
  const long i = (blk0 + blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int lane = threadIdx.x & 63;
  const bool ki = state[i] > 0;
  const long k1 = rowptr[i + 1];
  const unsigned long long key_i = prio ? prune_key(prio[i]) : 0ull, want_i = !KEY && prio && !ki ? key[i] : 0ull;
  unsigned long long best_key = kPruneNoKey;
  int best = kPruneNoOwner;
  for (long k = rowptr[i] + lane; k < k1; k += 64) {
    const int j = col[k];
    const bool kj = state[j] > 0;
    if (ki == kj) continue;
    if (ki) {                                                // i kept, j dropped
      if constexpr (KEY) atomicMin(&key[j], key_i);
      else if (!prio || key[j] == key_i) atomicMin(&owner[j], (int)i);
    } else {                                                 // j kept, i dropped
      if constexpr (KEY) best_key = min(best_key, prune_key(prio[j]));
      else if (!prio || prune_key(prio[j]) == want_i) best = min(best, j);
    }
  }
  if (ki) return;                                            // wave-uniform
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    if constexpr (KEY) best_key = min(best_key, (unsigned long long)__shfl_xor((long long)best_key, off));
    else best = min(best, __shfl_xor(best, off));
  }
  if (lane == 0) {
    if constexpr (KEY) { if (best_key != kPruneNoKey) atomicMin(&key[i], best_key); }
    else if (best != kPruneNoOwner) atomicMin(&owner[i], best);
  }
}

// the checks of a caller's CSR on the device: rowptr first (bad |= 1), and only behind a sound rowptr -- every range then lies inside [0, rowptr[n]), the
// length the caller vouches for -- the columns, one wave per row (bad |= 2)
__global__ void __launch_bounds__(256) k_ld_prune_check_rowptr(const long *__restrict__ rowptr, long n, int *__restrict__ bad) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n && ((i == 0 && rowptr[0] != 0) || rowptr[i + 1] < rowptr[i])) atomicOr(bad, 1);
}
__global__ void __launch_bounds__(256) k_ld_prune_check_col(const long *__restrict__ rowptr, const int *__restrict__ col, long n, int *__restrict__ bad, long blk0) {
  if (*bad) return;
  const long i = (blk0 + blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const long k0 = rowptr[i], k1 = rowptr[i + 1];
  for (long k = k0 + (threadIdx.x & 63); k < k1; k += 64) {
    const long j = col[k];
    if (j <= i || j >= n || (k > k0 && col[k - 1] >= j)) atomicOr(bad, 2);
  }
}
__global__ void __launch_bounds__(256) k_ld_prune_check_nan(const double *__restrict__ prio, long n, int *__restrict__ bad) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n && prio[i] != prio[i]) atomicOr(bad, 4);
}

static int prune_need(const char *who, size_t bytes) {
  size_t free_b = 0, total_b = 0;
  MXA_HIP(hipMemGetInfo(&free_b, &total_b));
  if (bytes > free_b) { set_error(12, "%s: not enough device memory: required %zu GB, free %zu GB", who, bytes >> 30, free_b >> 30); return 1; }
  return 0;
}
// what ld_prune_graph allocates: state, rm, bl; the owner pass's keys; the device copies of host outputs; the counters
static size_t prune_graph_bytes(long snps, bool with_owner, bool with_prio, bool out_dev) {
  const size_t n = (size_t)snps;
  return 3 * sizeof(int) * n + (with_owner && with_prio ? sizeof(unsigned long long) * n : 0) + (out_dev ? 0 : n + (with_owner ? sizeof(int) * n : 0)) + 4096;
}

// priority on the device and free of NaN: *d_prio = the caller's device pointer, or an upload into `tmp`; nullptr stays nullptr
static int prune_priority(const char *who, long snps, const double *priority, XBuf &tmp, XBuf &d_bad, hipStream_t s, const double **d_prio) {
  *d_prio = priority;
  if (!priority) return 0;
  if (ptr_location(priority, nullptr) == 1) {
    if (d_bad.alloc(sizeof(int))) return 1;
    MXA_HIP(hipMemsetAsync(d_bad.p, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_ld_prune_check_nan, dim3((unsigned)((snps + 255) / 256)), dim3(256), 0, s, priority, snps, (int *)d_bad.p);
    MXA_HIP(hipGetLastError());
    int bad = 0;
    MXA_HIP(hipMemcpyAsync(&bad, d_bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
    MXA_HIP(hipStreamSynchronize(s));
    if (bad) { set_error(1, "%s: priority holds a NaN", who); return 1; }
    return 0;
  }
  for (long i = 0; i < snps; i++)
    if (priority[i] != priority[i]) { set_error(1, "%s: priority[%ld] is NaN", who, i); return 1; }
  if (prune_need(who, sizeof(double) * (size_t)snps) || tmp.alloc(sizeof(double) * (size_t)snps)) return 1;
  MXA_HIP(hipMemcpyAsync(tmp.p, priority, sizeof(double) * (size_t)snps, hipMemcpyHostToDevice, s));
  *d_prio = (const double *)tmp.p;
  return 0;
}

// the checks of the outputs all three entries share; *out_dev: keep (and owner) are device pointers
static int prune_outputs(const char *who, const unsigned char *keep, const int *owner, bool *out_dev) {
  *out_dev = ptr_location(keep, nullptr) == 1;
  if (owner && (ptr_location(owner, nullptr) == 1) != *out_dev) { set_error(1, "%s: keep and owner must be both host or both device pointers", who); return 1; }
  return 0;
}

// The graph step on device arrays (d_prio may be nullptr, d_col too when the graph has no edge).  Every argument has been checked.
static int ld_prune_graph(const char *who, long snps, const long *d_rowptr, const int *d_col, const double *d_prio, unsigned char *keep, int *owner, bool out_dev,
                          long *n_kept, int *rounds, hipStream_t s) {
  const size_t n = (size_t)snps;
  if (prune_need(who, prune_graph_bytes(snps, owner != nullptr, d_prio != nullptr, out_dev))) return 1;
  XBuf d_state, d_cnt, d_key, d_keep, d_owner;               // d_state: state, rm, bl; d_cnt: kept (8 bytes), then the batch's undecided counts
  if (d_state.alloc(3 * sizeof(int) * n) || d_cnt.alloc(sizeof(unsigned long long) + sizeof(int) * kPruneBatchMax)) return 1;
  if (owner && d_prio && d_key.alloc(sizeof(unsigned long long) * n)) return 1;
  if (!out_dev && (d_keep.alloc(n) || (owner && d_owner.alloc(sizeof(int) * n)))) return 1;
  int *state = (int *)d_state.p, *rm = state + n, *bl = rm + n;
  unsigned long long *d_kept = (unsigned long long *)d_cnt.p;
  int *d_und = (int *)(d_kept + 1);
  unsigned char *r_keep = out_dev ? keep : (unsigned char *)d_keep.p;
  int *r_owner = !owner ? nullptr : out_dev ? owner : (int *)d_owner.p;
  MXA_HIP(hipMemsetAsync(state, 0, 3 * sizeof(int) * n, s));
  MXA_HIP(hipMemsetAsync(d_kept, 0, sizeof(unsigned long long), s));
  // One wave per row (edge and owner passes): 64 snps threads, 2^32 of them from 2^26 SNPs on, so these sweeps run in pieces (launch_in_block_chunks; the
  // pieces of a round read the states the round before left and write round stamps and atomic minima only, so their order does not matter).  One thread per
  // SNP in the vertex passes: snps is an int, a single launch.
  const long rows_blocks = (snps + 3) / 4;
  const dim3 vert_grid((unsigned)((snps + 255) / 256));
  int h_und[kPruneBatchMax];
  int round = 0, done = 0;
  for (int batch = kPruneBatch0; !done; batch = std::min(2 * batch, kPruneBatchMax)) {
    MXA_HIP(hipMemsetAsync(d_und, 0, sizeof(int) * (size_t)batch, s));
    for (int b = 0; b < batch; b++) {
      round++;
      const int *prev = b ? d_und + b - 1 : nullptr;
      launch_in_block_chunks(rows_blocks, [&](unsigned nb, long blk0) {
        hipLaunchKernelGGL(k_ld_prune_edges, dim3(nb), dim3(256), 0, s, d_rowptr, d_col, d_prio, snps, round, (const int *)state, rm, bl, prev, blk0);
      });
      hipLaunchKernelGGL(k_ld_prune_vertices, vert_grid, dim3(256), 0, s, snps, round, state, (const int *)rm, (const int *)bl, d_und + b, d_kept, prev);
    }
    MXA_HIP(hipGetLastError());
    MXA_HIP(hipMemcpyAsync(h_und, d_und, sizeof(int) * (size_t)batch, hipMemcpyDeviceToHost, s));
    MXA_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < batch && !done; b++)
      if (h_und[b] == 0) done = round - batch + b + 1;
  }
  hipLaunchKernelGGL(k_ld_prune_result, vert_grid, dim3(256), 0, s, snps, (const int *)state, r_keep, r_owner, (unsigned long long *)d_key.p);
  if (owner) {
    if (d_prio) launch_in_block_chunks(rows_blocks, [&](unsigned nb, long blk0) {
      hipLaunchKernelGGL(k_ld_prune_owner<true>, dim3(nb), dim3(256), 0, s, d_rowptr, d_col, d_prio, snps, (const int *)state, (unsigned long long *)d_key.p, r_owner, blk0);
    });
    launch_in_block_chunks(rows_blocks, [&](unsigned nb, long blk0) {
      hipLaunchKernelGGL(k_ld_prune_owner<false>, dim3(nb), dim3(256), 0, s, d_rowptr, d_col, d_prio, snps, (const int *)state, (unsigned long long *)d_key.p, r_owner, blk0);
    });
  }
  MXA_HIP(hipGetLastError());
  unsigned long long h_kept = 0;
  MXA_HIP(hipMemcpyAsync(&h_kept, d_kept, sizeof(h_kept), hipMemcpyDeviceToHost, s));
  if (!out_dev) {
    MXA_HIP(hipMemcpyAsync(keep, r_keep, n, hipMemcpyDeviceToHost, s));
    if (owner) MXA_HIP(hipMemcpyAsync(owner, r_owner, sizeof(int) * n, hipMemcpyDeviceToHost, s));
  }
  MXA_HIP(hipStreamSynchronize(s));
  *n_kept = (long)h_kept;
  if (rounds) *rounds = done;
  debug_info("%s: %ld of %ld SNPs kept in %d round(s)", who, (long)h_kept, snps, done);
  return 0;
}

static int ld_prune_csr(const char *who, long snps, const long *rowptr, const int *col, const double *priority, unsigned char *keep, int *owner, long *n_kept, int *rounds) {
  if (snps <= 0 || !rowptr || !keep || !n_kept) { set_error(1, "%s: bad arguments", who); return 1; }
  if (select_device() < 0) return 1;
  bool out_dev = false;
  if (prune_outputs(who, keep, owner, &out_dev)) return 1;
  XStream st;
  if (st.create(hipStreamDefault)) return 1;                 // blocking: ordered against the caller's default-stream work
  hipStream_t s = st.s;
  XBuf d_rp, d_cl, d_pr, d_bad, d_bad2;
  const size_t n = (size_t)snps;
  const bool rp_dev = ptr_location(rowptr, nullptr) == 1, cl_dev = ptr_location(col, nullptr) == 1;
  // rowptr: checked where it lies; a host copy of its last entry gives the number of pairs
  long nnz = 0;
  std::vector<long> h_rp;
  const long *h_rowptr = rowptr;
  if (rp_dev) {
    if (d_bad.alloc(sizeof(int))) return 1;
    MXA_HIP(hipMemsetAsync(d_bad.p, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_ld_prune_check_rowptr, dim3((unsigned)((snps + 255) / 256)), dim3(256), 0, s, rowptr, snps, (int *)d_bad.p);
    MXA_HIP(hipGetLastError());
    int bad = 0;
    MXA_HIP(hipMemcpyAsync(&bad, d_bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
    MXA_HIP(hipMemcpyAsync(&nnz, rowptr + snps, sizeof(long), hipMemcpyDeviceToHost, s));
    MXA_HIP(hipStreamSynchronize(s));
    if (bad) { set_error(1, "%s: rowptr needs rowptr[0] == 0 and must not decrease", who); return 1; }
    if (!cl_dev && nnz) {                                    // host columns under a device rowptr: the host check below wants the rows
      h_rp.resize(n + 1);
      MXA_HIP(hipMemcpy(h_rp.data(), rowptr, sizeof(long) * (n + 1), hipMemcpyDeviceToHost));
      h_rowptr = h_rp.data();
    }
  } else {
    if (rowptr[0] != 0) { set_error(1, "%s: rowptr[0] must be 0 (%ld)", who, rowptr[0]); return 1; }
    for (long i = 0; i < snps; i++)
      if (rowptr[i + 1] < rowptr[i]) { set_error(1, "%s: rowptr decreases at row %ld", who, i); return 1; }
    nnz = rowptr[snps];
  }
  if (nnz && !col) { set_error(1, "%s: bad arguments", who); return 1; }
  const long *d_rowptr = rowptr;
  const int *d_col = col;
  if (!rp_dev) {
    if (prune_need(who, sizeof(long) * (n + 1)) || d_rp.alloc(sizeof(long) * (n + 1))) return 1;
    MXA_HIP(hipMemcpyAsync(d_rp.p, rowptr, sizeof(long) * (n + 1), hipMemcpyHostToDevice, s));
    d_rowptr = (const long *)d_rp.p;
  }
  if (cl_dev && nnz) {
    if (!d_bad.p && d_bad.alloc(sizeof(int))) return 1;
    MXA_HIP(hipMemsetAsync(d_bad.p, 0, sizeof(int), s));
    launch_in_block_chunks((snps + 3) / 4, [&](unsigned nb, long blk0) {
      hipLaunchKernelGGL(k_ld_prune_check_col, dim3(nb), dim3(256), 0, s, d_rowptr, col, snps, (int *)d_bad.p, blk0);
    });
    MXA_HIP(hipGetLastError());
    int bad = 0;
    MXA_HIP(hipMemcpyAsync(&bad, d_bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
    MXA_HIP(hipStreamSynchronize(s));
    if (bad) { set_error(1, "%s: the columns of a row need i < col < snps, strictly ascending", who); return 1; }
  } else if (nnz) {
    for (long i = 0; i < snps; i++)
      for (long k = h_rowptr[i]; k < h_rowptr[i + 1]; k++)
        if (col[k] <= i || col[k] >= snps || (k > h_rowptr[i] && col[k - 1] >= col[k])) {
          set_error(1, "%s: the columns of a row need i < col < snps, strictly ascending (row %ld, col %d)", who, i, col[k]);
          return 1;
        }
    if (prune_need(who, sizeof(int) * (size_t)nnz) || d_cl.alloc(sizeof(int) * (size_t)nnz)) return 1;
    MXA_HIP(hipMemcpyAsync(d_cl.p, col, sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice, s));
    d_col = (const int *)d_cl.p;
  }
  const double *d_prio = nullptr;
  if (prune_priority(who, snps, priority, d_pr, d_bad2, s, &d_prio)) return 1;
  return ld_prune_graph(who, snps, d_rowptr, d_col, d_prio, keep, owner, out_dev, n_kept, rounds, s);
}

// The window entries: the pairs driver twice on device arrays of the library's own -- the count-only call sizes col exactly, the filling call writes col alone
// (no_val) -- and the graph step on them.  Neither the CSR nor a val array leaves the device; the second call's pre-flight sees rowptr and col allocated.
static int ld_prune_window(const char *who, const unsigned char *plink, long snps, long indiv, const int *last, double min_r2, const double *priority, unsigned char *keep,
                           int *owner, long *n_kept, int *rounds, bool pairwise, bool is_plink, const double *freq) {
  if (!plink || !last || !keep || !n_kept || snps <= 0 || indiv <= 0) { set_error(1, "%s: bad arguments", who); return 1; }
  if (select_device() < 0) return 1;
  bool out_dev = false;
  if (prune_outputs(who, keep, owner, &out_dev)) return 1;
  const size_t n = (size_t)snps;
  XBuf d_rp, d_cl, d_pr, d_bad;
  const double *d_prio = nullptr;
  long total = 0;
  {
    XStream st;                                              // the priority's check and upload; the pairs driver brings its own stream
    if (st.create(hipStreamDefault)) return 1;
    if (prune_priority(who, snps, priority, d_pr, d_bad, st.s, &d_prio)) return 1;
    MXA_HIP(hipStreamSynchronize(st.s));
  }
  const size_t graph = prune_graph_bytes(snps, owner != nullptr, priority != nullptr, out_dev);
  if (prune_need(who, sizeof(long) * (n + 1) + graph) || d_rp.alloc(sizeof(long) * (n + 1))) return 1;
  long *d_rowptr = (long *)d_rp.p;
  if (ld_pairs_any(who, plink, snps, indiv, last, min_r2, 1, d_rowptr, nullptr, nullptr, 0, &total, pairwise, is_plink, freq, true)) return 1;
  if (total) {
    if (prune_need(who, sizeof(int) * (size_t)total + graph) || d_cl.alloc(sizeof(int) * (size_t)total)) return 1;
    long again = 0;
    if (ld_pairs_any(who, plink, snps, indiv, last, min_r2, 1, d_rowptr, (int *)d_cl.p, nullptr, total, &again, pairwise, is_plink, freq, true)) return 1;
  }
  XStream st;
  if (st.create(hipStreamDefault)) return 1;
  return ld_prune_graph(who, snps, d_rowptr, total ? (const int *)d_cl.p : nullptr, d_prio, keep, owner, out_dev, n_kept, rounds, st.s);
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

// ---- the greedy selection on the pairs graph: the graph step alone, and the window entries (pairs driver + graph step, all on the device)
extern "C" int mxa_ld_prune_csr(int snps, const long *rowptr, const int *col, const double *priority, unsigned char *keep, int *owner, long *n_kept, int *rounds) {
  mxa::clear_error();
  return mxa::ld_prune_csr("mxa_ld_prune_csr", snps, rowptr, col, priority, keep, owner, n_kept, rounds);
}

extern "C" int mxa_ld_window_prune(const unsigned char *plink, int snps, int indiv, const int *last, double min_r2, const double *priority, unsigned char *keep, int *owner,
                                   long *n_kept, int *rounds, int is_plink_format, const double *allele_freq) {
  mxa::clear_error();
  return mxa::ld_prune_window("mxa_ld_window_prune", plink, snps, indiv, last, min_r2, priority, keep, owner, n_kept, rounds, false, is_plink_format != 0, allele_freq);
}

extern "C" int mxa_ld_window_prune_pairwise(const unsigned char *plink, int snps, int indiv, const int *last, double min_r2, const double *priority, unsigned char *keep,
                                            int *owner, long *n_kept, int *rounds) {
  mxa::clear_error();
  return mxa::ld_prune_window("mxa_ld_window_prune_pairwise", plink, snps, indiv, last, min_r2, priority, keep, owner, n_kept, rounds, true, true, nullptr);
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

extern "C" int snp_multiply_gpu(unsigned char *snp_matrix, int snps, int indiv, double *ans, bool is_plink_format) {
  // positional meaning as in the reference: arg 2 = packed (inner) dimension, arg 3 = output dimension
  mxa::clear_error();
  // MIRACULIX_NUM_GPUS = G > 1 with host operands: output-tile sharding inside this process (packed matrix replicated,
  // independent units, no collective).  Device g stages X itself, computes the column panel [c_g, c_g+1) of the symmetric result -- equal
  // numbers of 256-column tiles, which is equal work: a panel of t tile columns touches t * (rows / 256) tiles -- and downloads it over
  // its own PCIe link into the contiguous slab ans + c_g * indiv of the column-major host matrix.  Every tile is computed by the same
  // kernel as on one device, so the result is bit-identical.  Total work is the full matrix (2x the triangular single-device launch):
  // at config 3 the 80 GB download, not the arithmetic, bounds a host result, and that is what the G links divide.
  const int G = mxa::multi_requested();
  if (G > 1 && snp_matrix && ans && snps > 0 && indiv > 0 && mxa::ptr_location(snp_matrix, nullptr) == 0 && mxa::ptr_location(ans, nullptr) == 0) {
    const long nb = ((long)indiv + mxa::kXT - 1) / mxa::kXT;
    const int parts = (int)std::min<long>(G, nb);
    const int ndev = mxa_device_count();
    return mxa::run_on_devices(parts, [&](int g, int dev) {
      mxa::tl_xprod_shared_device = ndev > 0 && parts > ndev;   // worker threads are pooled: set on every job
      const long c0 = std::min<long>(indiv, nb * g / parts * mxa::kXT), c1 = std::min<long>(indiv, nb * (g + 1) / parts * mxa::kXT);
      if (c1 <= c0) return 0;
      return mxa::crossprod_any(snp_matrix, snps, indiv, ans + (size_t)c0 * indiv, is_plink_format, mxa::kPostNone, 0, nullptr, c0, c1, false, indiv, dev);
    });
  }
  return mxa::crossprod_any(snp_matrix, snps, indiv, ans, is_plink_format);
}

extern "C" int mxa_snp_multiply_panel(const unsigned char *snp_matrix, int snps, int indiv, int col_begin, int col_end, int upper_only, double *panel,
                                      long ld, int is_plink_format) {
  mxa::clear_error();
  return mxa::crossprod_any(snp_matrix, snps, indiv, panel, is_plink_format != 0, mxa::kPostNone, 0, nullptr, col_begin, col_end, upper_only != 0, ld);
}

extern "C" int mxa_grm(const unsigned char *plink_transposed, int snps, int indiv, double *G, int is_plink_format, int do_scale, const double *allele_freq) {
  mxa::clear_error();
  if (do_scale && !allele_freq) { mxa::set_error(1, "mxa_grm: allele frequencies are required when do_scale is set"); return 1; }
  return mxa::crossprod_any(plink_transposed, snps, indiv, G, is_plink_format != 0, mxa::kPostGrm, do_scale, allele_freq);
}

extern "C" int mxa_ld(const unsigned char *plink, int snps, int indiv, double *R, int is_plink_format, const double *allele_freq) {
  mxa::clear_error();
  if (!allele_freq) { mxa::set_error(1, "mxa_ld: allele frequencies are required"); return 1; }
  return mxa::crossprod_any(plink, indiv, snps, R, is_plink_format != 0, mxa::kPostLd, 0, allele_freq);
}
