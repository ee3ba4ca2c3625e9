// mxa_gemm_i8.hip -- OPT-IN engine (env MXA_ENGINE=i8): dgemm_compressed on the int8 matrix cores by exact slicing of B.
//
// Not the shipped default: the default path computes in fp64 on v_mfma_f64_4x4x4_4b_f64 (mxa_kernels.hip), as the reference
// does in fp64 FMAs.  This engine exploits that the genotype operand is an exact small integer (0,1,2).  Per column j, with E_j
// such that |b_kj| * 2^-E_j < 1/4, B is written in balanced radix 256:
//   b_kj * 2^-E_j = sum_{s<S} t_s / 2^(8(s+1)) + r,   t_s in [-128, 127],  |r| <= 0.502 * 2^(-8S)
// (computed exactly in integer arithmetic from the mantissa: sign-extended low byte, subtract, shift -- the digit set has no
// redundancy, so floating-point digit extraction would have to decide ties at the edge of the remainder range exactly).  Then
//   (Z B)_ij = sum_s 2^(E_j - 8(s+1)) * I_s,   I_s = sum_k z_ik t_s(k,j)     (exact int32 dot products on the int8 MFMA)
// -- the "Ozaki" error-free splitting of one operand; Z needs no splitting.  Entries far below the column maximum simply have
// zero leading digits, so nothing cancels in the recombination.  With S = 7 digits B is represented to 2^-54 of each column's
// largest entry; all integer sums are exact, only the final S-term fp64 combination rounds.  Error bound per output:
// 2 K * 2^(E_j - 57): at or below the rounding error of an fp64 dot product of that length for K = 1M, but it is a column-wise
// fixed-point representation, not element-wise fp64, so the engine stays opt-in and is never what bench.py reports.  For
// n <= 4 the kernel is HBM-bound with a single tile of 32 expanded columns, so the digits that fit the tile are free: n = 1 uses
// 32 digits (256 bits -- entries 60 decades below the column maximum still keep their whole mantissa), n = 2 uses 16.
//
// Kernel: one workgroup (4 waves, one per SIMD) per 256-row tile of the packed matrix and K range; wave tile 64 rows x
// (NT x 32) expanded columns (column e = slice * nc + j); accumulators NT x 2 tiles of v_mfma_i32_32x32x32_i8 (<= 256 AGPRs).
// Same LDS-DMA ring / mid-stage prefetch / unpack pipelining as k_crossprod2; A rows come from the tiled packed layout, the
// int8 slices of B are pre-arranged in MFMA fragment order by k_slice_B so every LDS read is a lane-linear ds_read_b128.
#include "mxa_internal.h"
#include "mxa_lds.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace mxa {

typedef int v16i __attribute__((ext_vector_type(16)));

// the packed genotype tiles come in by the non-temporal LDS-DMA (dma16_p<true>, mxa_lds.h: read once per pass), the digit slabs, which every row block
// re-reads, by the plain one
#ifndef MXA_NT_STREAM
#define MXA_NT_STREAM 1
#endif

// ---- slices in MFMA fragment order.  Bs[chunk][T][nt][lane][16]: T = K-step of 32 genotypes, nt = 32-wide tile of expanded
// columns e = s * nc + jj (slice s, column jj of the chunk), lane = (col = lane&31, h = lane>>5), byte 4q+i of the lane =
// digit of B[128(T/4) + 64h + 16(T%4) + 4i + q][chunk*nc + jj]: a lane of half h reads the 16 bytes (64 genotypes) 16h.. of its row
// per 128-genotype stage and uses dword T%4 of them in K-step T%4; unpack16 (mxa_lds.h) puts field 4i+q of that dword into byte i of register q.
// Balanced radix-256 digits of one double, exactly, in integer arithmetic.  b = +-m * 2^ex (m < 2^53 an integer).  In units of the
// last digit, 2^(E - 8S), the value is N = m * 2^p, p = ex - E + 8S: for p >= 0 the low p/8 digits are zero and the rest come from
// m << (p % 8); for p < 0 the bits below the last digit are rounded off (to nearest).  At most 9 digits are non-zero: they are packed
// into c[0..8] (least significant first) with d = sign-extended low byte, M = (M - d) >> 8 -- digits in [-128, 127], exact.
struct Digits9 { unsigned long long lo; unsigned int hi; int low_digits; };   // c[0..7] in lo, c[8] in hi; first digit position
__device__ __forceinline__ Digits9 balanced_digits(double b, int E, int S) {
  Digits9 d{0ull, 0u, 0};
  const long long bits = __double_as_longlong(b);
  const int ef = (int)((bits >> 52) & 0x7ff);
  long long m = bits & 0xfffffffffffffll;
  if (ef == 0x7ff || (ef == 0 && m == 0)) return d;            // non-finite columns are flagged separately; zero has no digits
  int ex;
  if (ef) { m |= 1ll << 52; ex = ef - 1075; } else ex = -1074;  // denormal input: no hidden bit
  const int p = ex - E + 8 * S;
  long long M;
  if (p >= 0) { d.low_digits = p >> 3; M = m << (p & 7); }
  else if (p <= -54) return d;                                  // entirely below the last digit
  else { const int sh = -p; M = (m + (1ll << (sh - 1))) >> sh; }
  if (bits < 0) M = -M;
#pragma unroll
  for (int i = 0; i < 8; i++) { const long long c = (long long)(signed char)(M & 0xff); d.lo |= (unsigned long long)(c & 0xff) << (8 * i); M = (M - c) >> 8; }
  d.hi = (unsigned int)(M & 0xff);                              // |M| <= 1 here: the last carry
  return d;
}
__device__ __forceinline__ unsigned int digit_of(const Digits9 &d, int S, int s) {   // digit of slice s (weight 2^(E - 8(s+1))) as a byte
  const int i = (S - 1 - s) - d.low_digits;
  if (i < 0 || i > 8) return 0u;
  return i < 8 ? (unsigned int)(d.lo >> (8 * i)) & 0xffu : d.hi;
}

// One pass over B for everything the guarded n <= 2 route needs to know about its columns (round 3; was four launches): per chunk c of a column
// the largest |entry| (inf if a non-finite one was seen), the smallest non-zero |entry|, and -- when centring -- sum b and sum f b.
// part[j*64 + c] = max, part[(n + j)*64 + c] = min; sums[(j*64 + c)*2 + {0, 1}].  Fixed thread -> row assignment and fixed trees: deterministic.
__global__ void __launch_bounds__(256) k_colstats_partial(const double *__restrict__ B, long ldb, long k, int n, const double *__restrict__ f, int want_sums,
                                                          double *__restrict__ part, double *__restrict__ sums) {
  const int j = blockIdx.y, c = blockIdx.x;
  const long per = (k + 63) / 64;
  const long c0 = c * per, c1 = c0 + per < k ? c0 + per : k;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  double mx = 0.0, lo = inf, s1 = 0.0, s2 = 0.0;
  // four rows of the thread per trip, all loads issued before the first use (round 6: a trip per row left the launch bound by the latency of ~15 dependent
  // trips, 8 us for 2 MB); the arithmetic keeps its order (rows ascending), so the partials are bit for bit what the one-row loop gave
  for (long r = c0 + threadIdx.x; r < c1; r += 4 * 256) {
    double bv[4], fv[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const long rr = r + (long)u * 256;
      const bool in = rr < c1;
      bv[u] = in ? B[rr + (long)j * ldb] : 0.0;
      fv[u] = (in && want_sums && f) ? f[rr] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (r + (long)u * 256 < c1) {
        const double b = bv[u], a = fabs(b);
        mx = (a <= 1.7976931348623157e308) ? fmax(mx, a) : inf;   // NaN counts as non-finite too (fmax would drop it)
        if (a > 0.0) lo = fmin(lo, a);
        if (want_sums) { s1 += b; if (f) s2 = fma(fv[u], b, s2); }
      }
  }
  __shared__ double sh[4][256];
  sh[0][threadIdx.x] = mx; sh[1][threadIdx.x] = lo; sh[2][threadIdx.x] = s1; sh[3][threadIdx.x] = s2;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      sh[0][threadIdx.x] = fmax(sh[0][threadIdx.x], sh[0][threadIdx.x + w]); sh[1][threadIdx.x] = fmin(sh[1][threadIdx.x], sh[1][threadIdx.x + w]);
      sh[2][threadIdx.x] += sh[2][threadIdx.x + w]; sh[3][threadIdx.x] += sh[3][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part[(size_t)j * 64 + c] = sh[0][0]; part[((size_t)n + j) * 64 + c] = sh[1][0];
    if (want_sums) { sums[((size_t)j * 64 + c) * 2] = sh[2][0]; sums[((size_t)j * 64 + c) * 2 + 1] = sh[3][0]; }
  }
}

// fused-final mode of k_slice_B (the guarded routes of n <= 6 and of peeled columns): every block derives the column exponents and the verdict of the
// exactness guard from the partials of k_colstats_partial itself (same data, same order: same answer in every block).  Round 5: the verdict is a CLASS,
// decided on the device so that no product waits for the host --
//   class 0: every column is represented exactly by S0 digits (the cheapest tile count for this n),  class 1: by S1 digits (one more tile; S1 = 0: no such
//   class),  class 2: neither (or a non-finite entry, or the recombination would leave the normal range): the fp64 kernel behind does the product.
// The chain of class c (this launch: my_class, my digits S) runs iff the class is c.  The publishing launch (the first chain's) writes for the kernels
// behind it: E, the column sums of the centring term, and three words  flags[0] = (class == 2), flags[1] = (class != 0), flags[2] = (class != 1)  -- so every
// later kernel keeps its one-word test (skip_if_set / run_if_set).  The words are WRITTEN, nobody has to clear them first.
struct SliceFused {
  const double *part; const double *sums;     // part == nullptr: legacy mode (E and the flag come from launch_colexp)
  int *E_out; int *flags_out; double *sumB, *sumfB;
  int bias, S0, S1, my_class, publish, want_sums;
};
constexpr int kSmallNMaxCols = 6;             // columns of a guarded small-n chain

// ---- fp64 chains BEHIND the guarded int8 chains (round 5): when the exactness verdict is class 2 the product is done in plain fp64 -- one thread per
// output row owns its dot products over the whole K range in ascending k: a plain FMA chain, the arithmetic of the reference
// (src/cuda/dgemm_compressed_cuda.h:259-266), deterministic, |error| <= K 2^-53 sum |z b|.  The work rides in the launch of k_slice_B (the publishing
// chain's): its blocks, which would return at once under that verdict, walk the output rows instead -- no launch of its own (the gated launch pairs /
// triples that stood here -- k_lut + k_finish; k_pack_B + k_gemm<MODE 0> + k_finish -- cost ~5 us each on a 1 ms product whether or not they ran).
// Plain form (tn = 0): thread <-> packed row, 32 bytes per slab of 128 genotypes; the entries of B are wave-uniform.
// Transposed-operand form (tn = 1): thread <-> individual (a packed column), one byte per packed row; K runs over the rows.
// n <= kSmallNMaxCols columns.  SLOW (measured late in round 5 on 500k x 50k: 44 ms ('T') / 198 ms ('N') at n = 4): since then only chains of ONE column use it (n = 1 and a peeled
// single column, where verdict class 2 needs inf / NaN or a span beyond 201 binades); wider chains are followed by gated launches of the fp64 kernels (mxa_product.cpp: guarded_small).
struct SmallNFallback {
  const uint8_t *G;                 // nullptr: no fallback in this launch
  long nslabs, m, k;
  double *C; long ldc, fill_rows;
  int tn, mode_trans, centered;
  const double *f;
};
__device__ __forceinline__ void small_n_fp64_row(const SmallNFallback &a, const double *__restrict__ B, long ldb, int n, long r, const double *sumB, const double *sumfB) {
  double v[kSmallNMaxCols];
#pragma unroll
  for (int j = 0; j < kSmallNMaxCols; j++) v[j] = 0.0;
  if (r < a.m) {
    if (!a.tn) {
      const uint8_t *row = a.G + (size_t)(r / kTileRows) * a.nslabs * kTileBytes + (size_t)(r % kTileRows) * kSlabBytes;
      for (long sl = 0; sl * kSlabK < a.k; sl++) {
        const uint4 w0 = *reinterpret_cast<const uint4 *>(row + (size_t)sl * kTileBytes), w1 = *reinterpret_cast<const uint4 *>(row + (size_t)sl * kTileBytes + 16);
        const uint32_t wd[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
        for (int d = 0; d < 8; d++) {
#pragma unroll
          for (int e = 0; e < 16; e++) {
            const long kk = sl * kSlabK + 16 * d + e;
            if (kk < a.k) {
              const double z = (double)((wd[d] >> (2 * e)) & 3u);
#pragma unroll
              for (int j = 0; j < kSmallNMaxCols; j++) if (j < n) v[j] = fma(z, B[kk + (long)j * ldb], v[j]);
            }
          }
        }
      }
    } else {
      // packed matrix rows = K; this thread's individual r: byte (r % 128) / 4 of slab r / 128, field r % 4
      const uint8_t *col = a.G + (size_t)(r / kSlabK) * kTileBytes + (size_t)(r % kSlabK) / 4;
      const int sh = 2 * (int)(r & 3);
      for (long t = 0; t * kTileRows < a.k; t++) {
        const uint8_t *tile = col + (size_t)t * a.nslabs * kTileBytes;
        const long rows = a.k - t * kTileRows < kTileRows ? a.k - t * kTileRows : kTileRows;
#pragma unroll 8
        for (long q = 0; q < rows; q++) {
          const double z = (double)((tile[q * kSlabBytes] >> sh) & 3u);
          const long kk = t * kTileRows + q;
#pragma unroll
          for (int j = 0; j < kSmallNMaxCols; j++) if (j < n) v[j] = fma(z, B[kk + (long)j * ldb], v[j]);
        }
      }
    }
    if (a.centered) {
#pragma unroll
      for (int j = 0; j < kSmallNMaxCols; j++) if (j < n) v[j] = a.mode_trans ? fma(-2.0 * sumB[j], a.f[r], v[j]) : v[j] + -2.0 * sumfB[j];
    }
  }
#pragma unroll
  for (int j = 0; j < kSmallNMaxCols; j++) if (j < n) a.C[r + (long)j * a.ldc] = v[j];   // rows [m, fill_rows): zeros
}

// tn_map (k_gemm_i8_tn): K-step T covers 32 consecutive K indices, byte 4q+i of lane (h, col) = digit of B[32 T + 16 h + 4 i + q]
__global__ void __launch_bounds__(256) k_slice_B(const double *__restrict__ B, long ldb, long k, int n, const int *__restrict__ E, int S, int nc, int NT,
                                                 long T_total, int ncols, uint32_t *__restrict__ Bs, long total, const int *__restrict__ skip_if_set,
                                                 SliceFused fu, int tn_map, SmallNFallback fb) {
  __shared__ int sE[kSmallNMaxCols], sflag, scls;
  __shared__ double sSum[2][kSmallNMaxCols];
  if (fu.part) {   // guarded small-n chain (n <= kSmallNMaxCols)
    if (threadIdx.x < 64) {
      int bad0 = 0, bad1 = 0;
      for (int j = 0; j < n; j++) {
        double m = fu.part[(size_t)j * 64 + threadIdx.x], lo = fu.part[((size_t)n + j) * 64 + threadIdx.x];
        double s1 = fu.want_sums ? fu.sums[((size_t)j * 64 + threadIdx.x) * 2] : 0.0, s2 = fu.want_sums ? fu.sums[((size_t)j * 64 + threadIdx.x) * 2 + 1] : 0.0;
        for (int o = 32; o > 0; o >>= 1) { m = fmax(m, __shfl_xor(m, o)); lo = fmin(lo, __shfl_xor(lo, o)); }
        if (fu.want_sums && fu.publish) {   // chunk sums in ascending chunk order, like k_colsum_final (every block: the fp64 rows below need them; block 0 publishes)
          double t1 = 0.0, t2 = 0.0;
          for (int c = 0; c < 64; c++) { t1 += __shfl(s1, c); t2 += __shfl(s2, c); }
          if (threadIdx.x == 0) { sSum[0][j] = t1; sSum[1][j] = t2; if (blockIdx.x == 0) { fu.sumB[j] = t1; fu.sumfB[j] = t2; } }
        }
        int e = 0;
        if (m > 0.0 && isfinite(m)) (void)frexp(m, &e);
        // exact with S digits iff the span e_max - e_min <= 8 S - 55 and the last digit's weight 2^(e_max + 2 - 8 S) stays normal (e_max >= 8 S - 1023)
        if (!isfinite(m)) { bad0 = 1; bad1 = 1; }
        else if (m > 0.0) {
          int el = 0; (void)frexp(lo, &el);
          if (!(e >= 8 * fu.S0 - 1023 && el >= e - (8 * fu.S0 - 55))) bad0 = 1;
          if (!(fu.S1 > 0 && e >= 8 * fu.S1 - 1023 && el >= e - (8 * fu.S1 - 55))) bad1 = 1;
        }
        if (threadIdx.x == 0) { sE[j] = e + fu.bias; if (fu.publish && blockIdx.x == 0) fu.E_out[j] = e + fu.bias; }
      }
      if (fu.S1 <= 0) bad1 = 1;
      if (threadIdx.x == 0) {
        const int cls = !bad0 ? 0 : !bad1 ? 1 : 2;
        sflag = cls != fu.my_class; scls = cls;
        // flags_out[-1] is the range flag of the denormal-operand mode (mxa_last_range_fallback): this product does not use that mode
        if (fu.publish && blockIdx.x == 0) { fu.flags_out[-1] = 0; fu.flags_out[0] = cls == 2; fu.flags_out[1] = cls != 0; fu.flags_out[2] = cls != 1; }
      }
    }
    __syncthreads();
    if (sflag) {
      if (fu.publish && scls == 2 && fb.G)   // not exact in any class: the fp64 chains, one thread per output row
        for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < fb.fill_rows; r += (long)gridDim.x * blockDim.x) small_n_fp64_row(fb, B, ldb, n, r, sSum[0], sSum[1]);
      return;
    }
    E = sE;
  } else if (skip_if_set && *skip_if_set) return;   // guarded route: B is not exactly representable, the fp64 fallback does this product
  // one thread per (q, column cj = chunk*nc + jj, h, T): reads the 4 values k = 128(T/4) + 64h + 16(T%4) + 4i + q (i = 0..3), writes dword q of
  // lane (h, col) for each slice.  q runs fastest, then the column: 16-byte lane records and 128-byte runs of doubles.
  // (Slice groups, round 6: with many digits per column (n = 1: 32) a thread walks all S slices -- 62 000 threads of ~1100 instructions each for the 250k-row
  // operand of a CG step, 11-12 us.  Four threads sharing the slices of one (q, column, h, K-step) took the 100k-row operand from 11.5 to 10 us and the 250k-row
  // one from 12 to 15 us, each deriving the digits of its four values again (profiles/r06_gram_step_kernel_timeline.txt): one thread stays.)
  for (long idx0 = (long)blockIdx.x * blockDim.x + threadIdx.x; idx0 < total; idx0 += (long)gridDim.x * blockDim.x) {
    const int q = (int)(idx0 & 3);
    const long rest = idx0 >> 2;
    const int cj = (int)(rest % ncols);
    const long hT = rest / ncols;
    const int h = (int)(hT & 1);
    const long T = hT >> 1;
    const int chunk = cj / nc, jj = cj % nc;
    Digits9 d[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const long kk = tn_map ? 32 * T + 16 * h + 4 * i + q : 128 * (T >> 2) + 64 * h + 16 * (T & 3) + 4 * i + q;   // K order of the A operand: see k_gemm_i8 / k_gemm_i8_tn
      d[i] = (kk < k && cj < n) ? balanced_digits(B[kk + (long)cj * ldb], E[cj], S) : Digits9{0ull, 0u, 0};
    }
    for (int s = 0; s < S; s++) {
      uint32_t w = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) w |= digit_of(d[i], S, s) << (8 * i);
      const int e = s * nc + jj;
      const int nt = e >> 5, col = e & 31;
      Bs[((((size_t)chunk * T_total + T) * NT + nt) * 64 + (size_t)(h * 32 + col)) * 4 + q] = w;
    }
  }
}

// ---- main kernel
constexpr int kI8Waves = 4;
constexpr int kI8StageK = 128;                    // genotypes per stage = one slab of the tiled layout
static_assert(kPlanTileRows == kTileRows && kPlanSlabK == kI8StageK && kPlanI8ABytes == kTileRows * kSlabBytes, "plan_i8 (mxa_plan.h) plans for these tiles");

template <int NT>
struct I8Cfg {
  static constexpr int kABytes = kTileRows * kSlabBytes;   // the rows of one packed tile: 8 KiB
  static constexpr int kBBytes = 4 * NT * 1024;   // 4 K-steps x NT tiles x 1 KiB
  static constexpr int kBufBytes = kABytes + kBBytes;
  // ring depth: as many stages as fit the 160 KiB LDS when one workgroup owns the CU (NT >= 5)
  // NT <= 4 needs at most 128 accumulator registers: two workgroups share a CU (3 buffers each) and hide each other's waits.
  static constexpr int kBufs = NT <= 4 ? 3 : 163840 / kBufBytes;
  static constexpr int kLds = kBufs * kBufBytes;
  static constexpr int kAUnits = kABytes / 1024;
  static constexpr int kUnits = kAUnits + 4 * NT;       // 1 KiB DMA units per stage
};

// scheduling pattern of one group of NM MFMAs: after MFMA i one LDS read (while i < NLOAD) and its share of the 7 unpack VALU
template <int I, int NM, int NLOAD>
struct SchedIter {
  static __device__ __forceinline__ void run() {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    if constexpr (I < NLOAD) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    constexpr int nv = 7 / NM + (I < 7 % NM ? 1 : 0);
    if constexpr (nv > 0) __builtin_amdgcn_sched_group_barrier(0x002, nv, 0);
    if constexpr (I + 1 < NM) SchedIter<I + 1, NM, NLOAD>::run();
  }
};

// Wave layout: WC waves side by side along the expanded columns, 4/WC along the rows; wave tile (MT x 32) rows x (NT/WC x 32)
// columns with MT * (4/WC) = 8 so that a workgroup covers one 256-row tile of the packed layout.
//   <NT, 2, 1>: every wave reads all NT B fragments per K-step (LDS read traffic 4 x NT KiB per K-step of 512 MFMA cycles)
//   <NT, 4, 2>: wave tile 128 x (NT/2 x 32): half the B-fragment LDS traffic, twice the unpack VALU (28 per 16 MFMAs)
// Direct finish (n <= 2, ONE K split, round 3): the workgroup holds the complete integer sums of its 256 rows, so it scales them, adds the digits
// of a column across the lanes in a fixed butterfly, applies the centring term and stores C itself -- no partial sums through HBM, no finish launch
// (the 'T' product of a CG step: 128 MB of int32 partials and ~25 us).  Same arithmetic as k_finish_i8_small up to the (fixed) order of the additions.
struct I8Direct {
  int on;                                   // 0: partial sums to P (finish kernel follows)
  const int *E; const double *colmax_part; double *C; long ldc; long m; long fill_rows;
  int n, S, nc, mode_trans, centered;
  const double *sumB, *sumfB, *f;
};

// (The unused pointer argument is the place of a diagnostic buffer that no launch ever passed.  It stays as padding: without it every argument behind it moves
// by 8 bytes, and on the one shape where the parent's five runs agreed to 0.15 % -- n = 1 'T', 250 000 x 100 000: 931.0-932.4 us -- the median came out at 934.7 us;
// with it the nine instantiations are the parent's machine code.  profiles/i8_fossils_refactor.txt)
template <int NT, int MT, int WC, bool SWAP1 = false>
__global__ void __launch_bounds__(256, 1)
k_gemm_i8(const uint8_t *__restrict__ G, size_t pitch, const int8_t *__restrict__ Bs, long T_total, int *__restrict__ P, long m_pad, int e_pad,
          int rowblocks, int nchunks, int stages_total, SplitTab tab, unsigned long long *__restrict__ /* unused */, const int *__restrict__ skip_if_set,
          I8Direct dir) {
  constexpr int ROWS = MT * (4 / WC) * 32;             // rows this workgroup multiplies: one tile of the packed layout
  using Cfg = I8Cfg<NT>;
  if (skip_if_set && *skip_if_set) return;
  constexpr int NTW = NT / WC;
  static_assert(NT % WC == 0 && ROWS == kTileRows && MT * NTW <= 16, "wave tiling");
  // Operand roles (round 3).  The matrix cores draw less power when the FULL-entropy operand (the radix-256 digits) is the instruction's A and the
  // low-entropy one (genotype bytes 0..2) its B: a bare MFMA loop runs 4.17 Pop/s at 2.11 GHz that way round against 3.60 at 1.84 GHz the other
  // (tools/mfma_i8_probe3.hip), and from two tiles on this kernel is power-bound.  The fragments are symmetric (a lane holds 16 consecutive k of one
  // row / column), so swapping them just transposes the accumulator tile: lane & 31 = genotype row, registers = expanded column; the partial sums
  // then go to P TRANSPOSED, P[split][e][row] (rows along the lanes: 128-byte runs), and k_finish_i8_t reads them that way.
  // (SWAP1: the one-tile launch of a product with three or more columns -- no in-kernel finish, no k_finish_i8_small -- stores transposed like the wider ones,
  // so that k_finish_i8_t finishes it: 36 us where a row-major general finish, since removed, took 77 behind a 500k-row product)
  constexpr bool kSwap = NT >= 2 || SWAP1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave / WC, wc = wave % WC;
  // XCD-aware order as in k_gemm: the row blocks of one (chunk, split) group stream the same digit slabs; whole groups (the first
  // 8 * floor(groups / 8)) are dealt to the 8 XCDs, blockIdx.x & 7 = XCD, so a group's slabs cross the fabric once
  const int bid = blockIdx.x;
  const int ngroups = (int)(gridDim.x / rowblocks), g8 = ngroups & ~7;
  int rb, grp;
  if (bid < g8 * rowblocks) { const int xcd = bid & 7, slot = bid >> 3; rb = slot % rowblocks; grp = xcd + 8 * (slot / rowblocks); }
  else { const int t = bid - g8 * rowblocks; rb = t % rowblocks; grp = g8 + t / rowblocks; }
  const int nc = grp % nchunks;
  const int sp = grp / nchunks;
  const int st0 = tab.begin[sp], st1 = tab.begin[sp + 1];
  const int stages = st1 - st0;
  const uint32_t lds0 = (uint32_t)(size_t)(lptr_t)smem;
  const uint32_t v_lane = lane * 16;
  const char *A_u = reinterpret_cast<const char *>(G) + (size_t)rb * (pitch / kSlabBytes) * kTileBytes;
  const char *B_u = reinterpret_cast<const char *>(Bs) + (size_t)nc * ((size_t)T_total * NT * 1024);

  // (with several column chunks -- the opt-in engines at wide n -- a packed tile is an operand of every chunk; choosing the policy per launch with a
  // wave-uniform branch around the DMA issue cost those power-bound launches 4 % (the branch splits the stage's basic block), the hint itself < 1 %: it stays)
  auto issue = [&](int stage, int buf) {   // stage index relative to st0
    const uint32_t base = lds0 + buf * Cfg::kBufBytes;
    const char *asrc = A_u + (size_t)(st0 + stage) * kTileBytes;
    const char *bsrc = B_u + (size_t)(st0 + stage) * ((size_t)4 * NT * 1024);
#pragma unroll
    for (int i = 0; i < (Cfg::kUnits + kI8Waves - 1) / kI8Waves; i++) {
      const int u = wave + i * kI8Waves;
      if (Cfg::kUnits % kI8Waves == 0 || u < Cfg::kUnits) {
        if (u < Cfg::kAUnits) dma16_p<MXA_NT_STREAM != 0>(asrc + u * 1024, v_lane, base + u * 1024);
        else dma16_s(bsrc + (u - Cfg::kAUnits) * 1024, v_lane, base + Cfg::kABytes + (u - Cfg::kAUnits) * 1024);
      }
    }
  };

  v16i acc[MT][NTW];
#pragma unroll
  for (int a = 0; a < MT; a++)
#pragma unroll
    for (int b = 0; b < NTW; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[a][b][r] = 0;

  const int a_off = (wr * (MT * 32) + (lane & 31)) * kSlabBytes + (lane >> 5) * 16;
  const int b_off = Cfg::kABytes + (wc * NTW) * 1024 + lane * 16;

  constexpr int NB = Cfg::kBufs;
  constexpr int kPerWave = Cfg::kUnits / kI8Waves;     // 2 + NT DMAs per wave and stage
  static_assert(Cfg::kUnits % kI8Waves == 0 && (NB - 2) * kPerWave < 64, "vmcnt bookkeeping");
  // Ring of NB buffers.  At the middle of stage s every wave has finished stage s-1, so that buffer takes stage s+NB-1; stage s+1 is
  // waited for there (stages s+2 .. s+NB-2 stay in flight) and its packed A words are prefetched into registers.  B fragments are
  // read from LDS one K-step ahead of their use, so the buffer of stage s stays live until the stage ends.
#pragma unroll
  for (int i = 0; i < NB - 1; i++) if (i < stages) issue(i, i);
  if (stages >= NB - 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NB - 2) * kPerWave) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  uint4 aw[MT], awn[MT];
#pragma unroll
  for (int a = 0; a < MT; a++) { aw[a] = *reinterpret_cast<const uint4 *>(smem + a_off + a * 32 * kSlabBytes); awn[a] = aw[a]; }
  int buf = 0;
  auto comp = [](const uint4 &w, int c) -> uint32_t { return c == 0 ? w.x : c == 1 ? w.y : c == 2 ? w.z : w.w; };
  v4i af_cur = unpack16(aw[0].x);
  v4i bf_cur[NTW], bf_nxt[NTW];
#pragma unroll
  for (int b = 0; b < NTW; b++) { bf_cur[b] = *reinterpret_cast<const v4i *>(smem + b_off + b * 1024); bf_nxt[b] = bf_cur[b]; }
  for (int s = 0; s < stages; s++) {
    const char *bbase = smem + buf * Cfg::kBufBytes + b_off;
    const int nb = buf == NB - 1 ? 0 : buf + 1;
    const char *bnext = smem + (s + 1 < stages ? nb : buf) * Cfg::kBufBytes + b_off;
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
      if (ks == 2 && s + 1 < stages) {
        if (s + NB - 2 < stages) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NB - 3) * kPerWave) : "memory");   // stage s+1 has landed
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (s + NB - 1 < stages) issue(s + NB - 1, buf == 0 ? NB - 1 : buf - 1);
#pragma unroll
        for (int a = 0; a < MT; a++) awn[a] = *reinterpret_cast<const uint4 *>(smem + nb * Cfg::kBufBytes + a_off + a * 32 * kSlabBytes);
      }
      // B fragments of the next K-step (after ks = 3: of the next stage, landed and visible since the barrier above; in the very
      // last K-step the current buffer is re-read and the values are never used).  The reads and the unpack VALU are pinned
      // between the MFMAs (sched_group_barrier): left alone the compiler sinks the reads to just before their first use and
      // clusters the VALU, which exposes the LDS latency in every K-step.
      const char *bsrc = ks < 3 ? bbase + (ks + 1) * NT * 1024 : bnext;
#pragma unroll
      for (int a = 0; a < MT; a++) {
        const uint32_t wa = a < MT - 1 ? comp(aw[a + 1], ks) : (ks < 3 ? comp(aw[0], ks + 1) : awn[0].x);
        const v4i af_nxt = unpack16(wa);
        const int lo = a * NTW / MT, hi = (a + 1) * NTW / MT;
#pragma unroll
        for (int b = 0; b < NTW; b++)
          if (b >= lo && b < hi) bf_nxt[b] = *reinterpret_cast<const v4i *>(bsrc + b * 1024);
#pragma unroll
        for (int b = 0; b < NTW; b++)
          acc[a][b] = kSwap ? __builtin_amdgcn_mfma_i32_32x32x32_i8(bf_cur[b], af_cur, acc[a][b], 0, 0, 0)
                            : __builtin_amdgcn_mfma_i32_32x32x32_i8(af_cur, bf_cur[b], acc[a][b], 0, 0, 0);
        SchedIter<0, NTW, (NTW + MT - 1) / MT>::run();
        __builtin_amdgcn_sched_barrier(0);
        af_cur = af_nxt;
      }
#pragma unroll
      for (int b = 0; b < NTW; b++) bf_cur[b] = bf_nxt[b];
    }
    buf = nb;
#pragma unroll
    for (int a = 0; a < MT; a++) aw[a] = awn[a];
  }

  // epilogue: P[split][row][e] int32, e contiguous: lanes (col) write 128-byte runs.  C/D map: col = lane&31,
  // row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
  const int col = lane & 31, rq = 4 * (lane >> 5);
  if (NT == 1 && WC == 1 && dir.on) {
    // lane = digit e = s * nc + jj of the rows it holds; weight 2^(E_jj - 8 (s + 1))
    const int sl = col / dir.nc, jj = col - sl * dir.nc;
    const bool live = col < dir.nc * dir.S;
    const int sh = live ? dir.E[jj] - 8 * (sl + 1) : 0;
    bool bad = false;
    double cs = 0.0;
    if (col < dir.nc && col < dir.n) {
      double cm = 0.0;
      for (int c = 0; c < 64; c++) cm = fmax(cm, dir.colmax_part[(size_t)col * 64 + c]);
      bad = !(cm <= 1.7976931348623157e308);   // a column with inf / NaN: NaN, like 0 * inf in fp64
      if (dir.centered) cs = -2.0 * (dir.mode_trans ? dir.sumB[col] : dir.sumfB[col]);
    }
#pragma unroll
    for (int a = 0; a < MT; a++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const long row = (long)rb * ROWS + wr * (MT * 32) + a * 32 + (r & 3) + 8 * (r >> 2) + rq;
        double v = live ? ldexp((double)acc[a][0][r], sh) : 0.0;
        // the 32 lanes of a half-wave hold the digits of one row; lanes of one column: e = jj, jj + nc, ...  (nc = 1: all 32; nc = 2: equal parity)
        for (int off = 16; off >= dir.nc; off >>= 1) v += __shfl_xor(v, off, 32);
        if (col < dir.nc && col < dir.n && row < dir.m) {
          if (bad) v = __longlong_as_double(0x7ff8000000000000ll);
          if (dir.centered) v = dir.mode_trans ? fma(cs, dir.f[row], v) : v + cs;
          dir.C[row + (long)col * dir.ldc] = v;
        }
      }
    if (rb == rowblocks - 1)   // rows [m, fill_rows) of every column are zero (ld padding of the plain ABI), whatever the tile padding
      for (long r = dir.m + threadIdx.x; r < dir.fill_rows; r += 256)
        for (int c = 0; c < dir.n; c++) dir.C[r + (long)c * dir.ldc] = 0.0;
    return;
  }
  int *Pb = P + (size_t)sp * m_pad * e_pad;
  if (kSwap) {
#pragma unroll
    for (int a = 0; a < MT; a++)
#pragma unroll
      for (int b = 0; b < NTW; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const long row = (long)rb * ROWS + wr * (MT * 32) + a * 32 + col;
          const int e = nc * (NT * 32) + (wc * NTW + b) * 32 + (r & 3) + 8 * (r >> 2) + rq;
          Pb[(size_t)e * m_pad + row] = acc[a][b][r];
        }
    return;
  }
#pragma unroll
  for (int a = 0; a < MT; a++)
#pragma unroll
    for (int b = 0; b < NTW; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const long row = (long)rb * ROWS + wr * (MT * 32) + a * 32 + (r & 3) + 8 * (r >> 2) + rq;
        Pb[(size_t)row * e_pad + (size_t)nc * (NT * 32) + (wc * NTW + b) * 32 + col] = acc[a][b][r];
      }
}

// ---- transposed-operand form for n <= 2 (round 4): C (indiv x n) = Zc B computed from the SNP-MAJOR copy, i.e. K runs over the packed matrix's ROWS and the
// output runs along its packed direction -- the kernel single-orientation storage needs for the 'N' product of the CG step.
// MFMA roles: A = the digits (M = the 32 expanded columns e = s * nc + jj, K = 32 SNPs), B = genotypes (N = 32 individuals, K = 32 SNPs); D[e][individual].
// The B operand needs, per lane, 16 consecutive SNPs of ONE individual as bytes, while a packed dword holds 16 individuals of one SNP: lane (cg, khalf)
// loads the 16 dwords W[r] = column group cg (16 individuals) of SNP rows 16 khalf + r, gathers bytes with 8 v_perm_b32 per four rows (P[q][b]: byte i =
// byte b of W[4 i + q]) and masks the four 2-bit fields of every byte WHERE THEY STAND (field g of byte b = individual 4 b + g, scaled by 4^g; the top
// field is shifted down by 2, scale 16): R[f][q] is the operand of individual 16 cg + f, and MFMA number f of the K-step multiplies the 32 individuals
// {16 cg + f}.  112 VALU per 16 MFMAs and 256 genotypes per lane -- 0.44 per genotype, what the plain unpack costs.  The accumulator of MFMA f carries
// the scale 4^min(f & 3, 2) * (f & 3 == 3 ? 4 : 1); it is divided out (exact shift) when the partial sums are stored.
// Workgroup (8 waves) = a strip of 512 individuals (4 slabs) x a range of row blocks (256 SNPs each); four wave pairs split the 8 K-steps of a row block,
// the two waves of a pair split the 16 MFMA groups; the accumulators are added at the end through LDS.  LDS image of a stage: [slab j][K-step][32 rows x 32 B], slab regions 64 B apart modulo the bank period and rows
// 16..31 of every unit rotated by one row (done on the GLOBAL side of the lane-linear DMA), so that the 64 lanes of a W load hit 64 different banks
// (bank = dword of the column group (8) + 8 * khalf + 16 * slab).
// Partial sums go to P[split][e][individual] like the operand-swapped plain instantiations: k_finish_i8_t finishes them (exact int64 over the splits).
constexpr int kTnSlabStride = kTileBytes + 64;                // LDS bytes between the slab regions of a stage
#ifndef MXA_TN_WAVE_LOCAL
#define MXA_TN_WAVE_LOCAL 1                                   // 0: A/B build of the round-5 form (workgroup barrier per stage)
#endif

// Workgroup = a strip of 256 individuals (2 slabs) x a range of row blocks, 4 waves.  Only 16 column groups exist, so the byte-pair split sits in the lanes:
// lane (cg = lane & 15, fh = (lane >> 4) & 1, khalf = lane >> 5) -- the two lanes of a column group read the same dword (an LDS broadcast) and gather
// different byte pairs (the v_perm selector is per lane); MFMA group j multiplies the individuals 16 cg + 8 fh + j.  Wave w: K-steps {2 w, 2 w + 1}.
// (The first version -- 512 individuals, 8 waves, one workgroup per CU -- was no faster and was removed in round 5.)
// Round 5: the digit fragments no longer pass through LDS.  A wave needs 2 KiB of them per stage (its two K-steps; the same for every strip, L2-resident):
// each lane loads its 2 x 16 bytes straight into registers, BUFS - 1 stages ahead like the packed tiles.  A stage's LDS buffer shrinks from 24 to 16 KiB, so
// the ring holds BUFS - 1 = 3 stages in flight per workgroup (was 2) with two workgroups per CU: 96 KiB of packed bytes on their way per CU instead of 64 --
// the kernel is bound by the packed stream's latency, not by its arithmetic (DMA ring alone: 0.93 ms where the full kernel took 1.03, profiles/r04).
constexpr int kTnSlabs = 2;
// (which pieces of which strips a workgroup multiplies: TnSched, mxa_plan.h -- host-only code, swept on the CPU)
template <int BUFS, int TT>
struct TnCfg {
  static constexpr int kWaves = 4;
  static constexpr int kBufBytes = kTnSlabs * kTnSlabStride;        // packed rows of one stage: 2 slabs x 8 KiB (+ the bank offset)
  static constexpr int kLds = BUFS * kBufBytes < 4 * 8192 ? 4 * 8192 : BUFS * kBufBytes;   // at least the 32 KiB of the final reduction
  static constexpr int kPackedPerWave = kTnSlabs * 8 / kWaves;      // 4 DMA units per wave and stage
  static constexpr int kOpsPerWave = kPackedPerWave + 2 * TT;       // + the wave's digit loads (two K-steps x TT tiles): what vmcnt counts per stage
  static constexpr int kDepth = BUFS - 1;                           // stages in flight
};
// TT = digit tiles (32 expanded columns each) per pass over the matrix.  TT = 1: n <= 2, peeled columns, n = 3 with few digits -- 128 accumulator registers,
// two workgroups per CU, 4 buffers.  TT = 2 (round 5): 3 <= n <= 6 -- the byte gather of a K-step feeds the MFMAs of BOTH tiles, 256 accumulator registers,
// one workgroup per CU (one wave per SIMD), 6 buffers = 5 stages in flight to cover the latency alone: ONE pass where round 4 took two.

template <int BUFS, int TT>
__global__ void __launch_bounds__(256, TT == 1 ? 2 : 1)
k_gemm_i8_tn(const uint8_t *__restrict__ G, long nslabs_all, const int8_t *__restrict__ Ad, int digit_tiles, int *__restrict__ P, long m_pad, int e_pad, int e_off,
             TnSched sc, const int *__restrict__ skip_if_set) {
  // Ad: the digit fragments of THIS launch's tile of 32 expanded columns, K-steps digit_tiles KiB apart (k_slice_B interleaves the tiles of a K-step);
  // the sums go to rows e_off .. e_off + 31 of P[split][e_pad][m_pad].  A product with several tiles (3 <= n <= 6, the opt-in engines) is one launch per tile.
  using Cfg = TnCfg<BUFS, TT>;
  constexpr int D = Cfg::kDepth, NSET = D + 1;
  constexpr bool kWaveLocal = MXA_TN_WAVE_LOCAL && TT == 1;   // every wave fetches the DMA units it consumes: no workgroup barrier per stage (issue_packed)
  if (skip_if_set && *skip_if_set) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fh = (lane >> 4) & 1;                             // field half
  const uint32_t lds0 = (uint32_t)(size_t)(lptr_t)smem;
  // PERSISTENT workgroups over ITEMS = (strip, piece of its K range) (round 5).  Integer sums are exact, so the result does not depend on where the cuts
  // fall -- which frees them; a slot is never re-dispatched (a replaced workgroup cost ~10 us of idle slot).  The schedule is TnSched's (mxa_plan.h), either
  // mode 0 -- strips cut into c or c + 1 equal pieces such that the items fill whole rounds of the resident slots (391 strips x 5 equal splits on 512 slots took
  // 4 rounds for 3.82 rounds of work; 298 strips x 5 + 93 x 6 pieces take 3 rounds of 195 stages + 1 of 163); the items of a round start together and sweep
  // their K ranges in step, so the digit fragments they share stay in the L2s (an even cut of the strip-major stage sequence, tried first, scattered the
  // workgroups over all row blocks: 1.20 ms against 1.04) -- or mode 1 (round 6): heads [0, la) of the strips on one class of workgroups, the tails dealt
  // evenly to the others: 2.3 pieces per strip instead of 5.2, and every piece is 32 KiB of sums leaving for HBM.  A piece's sums go to P[slot][e][individual].
  int strip = 0, st0 = 0, stages = 0, slot = 0;
  // DMA: LDS granule `lane` of a packed unit takes the global granule sigma(lane): rows 16..31 land rotated by one row
  const int rho = (lane - 32) >> 1;
  const uint32_t v_pack = lane < 32 ? (uint32_t)lane * 16 : (uint32_t)(2 * (16 + ((rho + 15) & 15)) + (lane & 1)) * 16;
  const uint32_t v_lin = (uint32_t)lane * 16;
  // all global traffic of one stage: 4 packed DMA units, then the two digit loads (asm: the compiler does not see the DMA, so it must not count vmcnt either)
  auto issue_packed = [&](int stage, int buf) {               // stage relative to st0
    const uint32_t base = lds0 + buf * Cfg::kBufBytes;
    const size_t rb = (size_t)(st0 + stage);
#pragma unroll
    for (int i = 0; i < Cfg::kPackedPerWave; i++) {
      // Round 6, one-tile instantiation (TT = 1; two workgroups per CU): a wave fetches exactly the units it consumes -- K-steps 2 wave, 2 wave + 1 of both slabs -- so no
      // other wave ever touches its part of the ring and the stage loop needs NO workgroup barrier: the wave's own vmcnt orders its DMA against its LDS reads.
      // Measured on one box, alternating with the round-5 form (units dealt wave + 4 i, __syncthreads per stage; profiles/r06_tn_wave_local_ab.txt): n = 1 0.986 / 1.003 ms
      // against 0.991 / 1.015, n = 2 and 3 equal within the noise -- a small gain; the TWO-tile instantiation (one workgroup per CU) LOSES 6-13 % without the barrier
      // (n = 4: 1.60 against 1.41 ms: four waves drifting apart turn the stage's 16 KiB burst into 4 KiB requests) and keeps the lockstep form.
      static_assert(kTnSlabs == 2 && Cfg::kWaves == 4 && Cfg::kPackedPerWave == 4, "wave-local DMA units: 2 slabs x 2 K-steps per wave");
      const int u = kWaveLocal ? (i >> 1) * 8 + 2 * wave + (i & 1) : wave + i * Cfg::kWaves;       // slab j = u >> 3, K-step u & 7
      long sl = (long)strip * kTnSlabs + (u >> 3);
      if (sl >= nslabs_all) sl = nslabs_all - 1;             // individuals beyond the matrix: rows of P nobody reads
      dma16_p<MXA_NT_STREAM != 0>(reinterpret_cast<const char *>(G) + (rb * (size_t)nslabs_all + (size_t)sl) * kTileBytes + (u & 7) * 1024, v_pack, base + (u >> 3) * kTnSlabStride + (u & 7) * 1024);
    }
  };
  auto issue_digits = [&](int stage, v4i (&d)[2][TT]) {       // the tiles of a K-step are 1 KiB apart, the K-steps digit_tiles KiB
    const char *src = reinterpret_cast<const char *>(Ad) + ((size_t)(st0 + stage) * 8 + (size_t)(2 * wave)) * ((size_t)digit_tiles * 1024);
#pragma unroll
    for (int kk = 0; kk < 2; kk++)
#pragma unroll
      for (int tt = 0; tt < TT; tt++)
        asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(d[kk][tt]) : "v"(v_lin), "s"(src + (size_t)kk * digit_tiles * 1024 + (size_t)tt * 1024) : "memory");
  };
  v16i acc[8][TT];
  const int cg = lane & 15, khalf = lane >> 5;
  // byte offset of W[r] inside a packed unit: slab region + row position (rotated for the upper half) * 32 + dword of the column group.  Row position of
  // W[r]: r (lower K half) or 16 + ((r + 1) & 15) (upper half) = 17 + r for r < 15: ONE per-lane base + r * 32 as an immediate serves r = 0 .. 14 of both
  // halves, W[15] (row 15 / row 16) has its own (two address registers instead of sixteen: the two-tile instantiation holds 256 accumulators)
  const int w_base = (cg >> 3) * kTnSlabStride + (khalf ? 17 : 0) * kSlabBytes + (cg & 7) * 4;
  const int w_15 = (cg >> 3) * kTnSlabStride + (khalf ? 16 : 15) * kSlabBytes + (cg & 7) * 4;
  const uint32_t sel1 = fh ? 0x07030602u : 0x05010400u;     // first gather stage: byte pairs (2 fh, 2 fh + 1) of the two rows

  int item_i = 0;
  int tail_g = 0;
  TnItem item;
  while (tn_next(sc, (int)blockIdx.x, item_i, tail_g, item)) {
  {
  // ---- one item: stages [st0, st0 + stages) of `strip`
  strip = __builtin_amdgcn_readfirstlane(item.strip); st0 = __builtin_amdgcn_readfirstlane(item.st0);
  stages = __builtin_amdgcn_readfirstlane(item.stages); slot = __builtin_amdgcn_readfirstlane(item.slot);
#pragma unroll
  for (int f = 0; f < 8; f++)
#pragma unroll
    for (int tt = 0; tt < TT; tt++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[f][tt][r] = 0;
  // digit fragments of this wave's two K-steps (x TT tiles), one register set per stage in flight (+ the one in use).  Declared and cleared PER ITEM: as values
  // that live from one item to the next they crossed the epilogue, were spilled there (two tiles: all 256 registers are accumulators), and the compiler's own
  // waits for those scratch accesses -- vmcnt(0..5), counted without the DMA it does not see -- landed in the stage loop: 1.86 ms where 1.45 had been measured.
  v4i dig[NSET][2][TT];
#pragma unroll
  for (int i = 0; i < NSET; i++)
#pragma unroll
    for (int kk = 0; kk < 2; kk++)
#pragma unroll
      for (int tt = 0; tt < TT; tt++) dig[i][kk][tt] = v4i{0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < D; i++) if (i < stages) { issue_packed(i, i); issue_digits(i, dig[i]); }
  for (int s0 = 0; s0 < stages; s0 += NSET) {
#pragma unroll
    for (int u = 0; u < NSET; u++) {
      const int s = s0 + u;
      if (s < stages) {
        // stage s has landed; the stages behind it (at most D - 1, fewer near the end: then everything is waited for) may be in flight
        if (s + D - 1 < stages) asm volatile("s_waitcnt vmcnt(%0)" : : "n"((D - 1) * Cfg::kOpsPerWave) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
        // (an empty volatile asm that "rewrites" the registers: volatile asms keep their order, so whatever reads the digits -- and any copy the register
        // allocator makes for this statement -- comes after the wait.  Tying the registers to the wait itself put such copies BEFORE it.)
#pragma unroll
        for (int kk = 0; kk < 2; kk++)
#pragma unroll
          for (int tt = 0; tt < TT; tt++) asm volatile("" : "+v"(dig[u][kk][tt]));
        // wave-local units: no barrier -- the wave is done with its own part of stage s - 1, whose buffer it refills now; otherwise: for every wave
        if (!kWaveLocal) __syncthreads();
        if (s + D < stages) { issue_packed(s + D, (s + D) % BUFS); issue_digits(s + D, dig[(u + D) % NSET]); }
        const char *bufp = smem + (s % BUFS) * Cfg::kBufBytes;
#pragma unroll
        for (int kk = 0; kk < 2; kk++) {
          const int T = 2 * wave + kk;                       // K-step of this wave inside the row block
          uint32_t W[16];
#pragma unroll
          for (int r = 0; r < 16; r++) W[r] = *reinterpret_cast<const uint32_t *>(bufp + T * 1024 + (r < 15 ? w_base + r * kSlabBytes : w_15));
          // byte gather, this lane's half: Pq[q][bb] byte i = byte (2 fh + bb) of W[4 i + q]
          uint32_t Pq[4][2];
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const uint32_t t = __builtin_amdgcn_perm(W[4 + q], W[q], sel1), v = __builtin_amdgcn_perm(W[12 + q], W[8 + q], sel1);
            Pq[q][0] = __builtin_amdgcn_perm(v, t, 0x05040100u); Pq[q][1] = __builtin_amdgcn_perm(v, t, 0x07060302u);
          }
#pragma unroll
          for (int f = 0; f < 8; f++) {
            const int bb = f >> 2, g = f & 3;
            v4i bf;
#pragma unroll
            for (int q = 0; q < 4; q++) bf[q] = (int)(g < 3 ? (Pq[q][bb] & (0x03030303u << (2 * g))) : ((Pq[q][bb] >> 2) & 0x30303030u));
#pragma unroll
            for (int tt = 0; tt < TT; tt++) acc[f][tt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(dig[u][kk][tt], bf, acc[f][tt], 0, 0, 0);
          }
        }
      }
    }
  }
  // ---- add the accumulators of the four waves that split the K-steps through LDS, two MFMA groups per pass, and store P[split][e][individual].
  // Round 6: the sums are collected in an LDS image of the strip's 32 x 256 block of P and leave as 16-byte-per-lane rows (a wave writes a whole 1 KiB row of one e per
  // instruction).  Until then every lane stored its 4-byte sums where they fell -- 64 lanes = 32 individuals 32 B apart in each of two rows per instruction, eight instructions
  // per cache line -- and the timing-only builds of this round showed what that cost: the kernel WITHOUT its partial-sum stores ran 0.92 ms where the whole one took 0.99-1.01
  // (no MFMAs, no byte gather, no LDS reads: no change; profiles/r06_tn_ablation.txt): 72 MB of stores were 8 % of a 6.3 GB kernel, because a workgroup streams nothing while
  // its epilogue drains.  The timing-only builds that followed (all items store into ONE 32 KiB region: 0.928 ms; no stores: 0.927; real: 1.017) showed that it is the
  // HBM write traffic itself, not the store pattern: the answer is fewer pieces (TnSched mode 1), and these rows stay because they are no slower and simpler to read.
  static_assert(Cfg::kLds >= 2 * 32768, "reduction buffer + the 32 x 256 image of P");
  __syncthreads();
  int *red = reinterpret_cast<int *>(smem);                  // [wave][group in pass (2)][reg (16)][lane (64)] ints = 8 KiB per wave
  int *img = reinterpret_cast<int *>(smem + 32768);          // [e (32)][individual of the strip (256)]
#pragma unroll
  for (int tt = 0; tt < TT; tt++) {
  int *Pb = P + ((size_t)slot * e_pad + e_off + 32 * tt) * m_pad;
#pragma unroll
  for (int pass = 0; pass < 4; pass++) {
#pragma unroll
    for (int gq = 0; gq < 2; gq++)
#pragma unroll
      for (int r = 0; r < 16; r++) red[((wave * 2 + gq) * 16 + r) * 64 + lane] = acc[pass * 2 + gq][tt][r];
    __syncthreads();
    {
      const int gq = wave & 1, r0 = 8 * (wave >> 1);         // this wave finishes group gq, registers r0 .. r0 + 7
      const int f = 8 * fh + 2 * pass + gq;                  // field of the dword = individual 16 cg + f
      const int sh = (f & 3) == 3 ? 4 : 2 * (f & 3);         // the in-place field scale of the group: 4^g, 16 for the top field
#pragma unroll
      for (int rr = 0; rr < 8; rr++) {
        const int r = r0 + rr;
        int v = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) v += red[((w * 2 + gq) * 16 + r) * 64 + lane];
        const int e = (r & 3) + 8 * (r >> 2) + 4 * khalf;
        img[e * 256 + 16 * cg + f] = v >> sh;                // exact: every product carried the factor
      }
    }
    __syncthreads();
  }
  // the image leaves: wave w writes rows e = 8 w .. 8 w + 7, lane l the individuals 4 l .. 4 l + 3 of the strip (m_pad is a multiple of the strip: 16-byte aligned)
  // (nontemporal: nobody reads them before the finish kernel -- 1.006-1.008 -> 0.983-0.984 ms on one box, profiles/r06_tn_nt_store.txt)
  {
    int *dst = Pb + (size_t)strip * (kTnSlabs * kSlabK) + 4 * lane;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int e = 8 * wave + i;
      __builtin_nontemporal_store(*reinterpret_cast<const v4i *>(img + e * 256 + 4 * lane), reinterpret_cast<v4i *>(dst + (size_t)e * m_pad));
    }
  }
  __syncthreads();                                           // (the next tile's sums / the next item's DMA reuse the image)
  }   // tiles of the pass
  }
  }   // items of this workgroup
}

// ---- finish: sum the splits exactly (int64), combine the slices smallest scale first, centring, ldc store.
// finish for the TRANSPOSED partial sums of the operand-swapped instantiations (NT >= 2): P[split][e][row], e = chunk * NT * 32 + s * nc + jj.
// One thread per (row, column): every load is a 1 KiB run along the rows, C is written along the rows: exact int64 sums over the splits, digits added
// smallest scale first.
// Block = 256 rows x 4 digit groups (round 4; was one thread per row walking all S digits and K splits in a chain of dependent loads: 100-170 us behind a
// 1 ms product).  Thread (lane, g) owns the digits s in [g Sg, (g + 1) Sg), Sg = ceil(S / 4) <= 8, of FOUR rows (lane, lane + 64, ...): all their partial
// sums over the K splits are loaded before the first use (rows along the lanes: 256-byte runs; one row per thread left the launch bound by the life
// time of its 47 000 short blocks: 81 us for 128 MB), added exactly (int64), scaled (exact) and added smallest scale first; the four groups of a row
// are then added smallest first through LDS -- a fixed order, at most Sg + 3 roundings per result.
constexpr int kFinTGroups = 4;
constexpr int kFinTRows = 4;                  // rows per thread
constexpr int kFinTBlockRows = 64 * kFinTRows;
__global__ void __launch_bounds__(256) k_finish_i8_t(const int *__restrict__ P, long m_pad, int e_pad, int splits, long m, int n, int S, int nc, int NT,
                                                     const int *__restrict__ E, const double *__restrict__ colmax_part, double *__restrict__ Cout, long ldc,
                                                     long fill_rows, int mode_trans, int centered, const double *__restrict__ sumB, const double *__restrict__ sumfB,
                                                     const double *__restrict__ f, const int *__restrict__ skip_if_set, int tn, TnSched tn_sc) {
  if (skip_if_set && *skip_if_set) return;
  // partial sums of the transposed-operand kernel (tn): this block's 256 rows are ONE strip of k_gemm_i8_tn; one slot of P per piece the schedule cut it into
  if (tn) splits = (long)blockIdx.x < tn_sc.strips ? tn_pieces(tn_sc, blockIdx.x) : 1;   // (blocks beyond the last strip: ld padding rows, zeros)
  const int j = blockIdx.y, chunk = j / nc, jj = j - chunk * nc;
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const long rbase = (long)blockIdx.x * kFinTBlockRows + lane;
  __shared__ int bad;
  __shared__ double part[kFinTGroups][kFinTBlockRows];
  if (threadIdx.x < 64) {   // wave 0: the column's largest |entry| from the 64 chunk maxima
    double cm = colmax_part[(size_t)j * 64 + lane];
    const bool nonfinite = !(cm <= 1.7976931348623157e308);
    const unsigned long long any = __ballot(nonfinite);
    if (lane == 0) bad = any != 0ull;            // column holds an inf or a NaN: the result column is NaN, like 0 * inf in fp64
  }
  const int Sg = (S + kFinTGroups - 1) / kFinTGroups, s0 = g * Sg;
  const int Ej = E[j];
  const int *p0 = P + (size_t)(chunk * (NT * 32) + jj) * m_pad;
  // rows clamped to valid addresses; every load of a digit pair is issued before the first use (few registers: eight waves per SIMD keep ~64 KiB per CU in flight)
  long rl[kFinTRows];
  double v[kFinTRows];
#pragma unroll
  for (int i = 0; i < kFinTRows; i++) { const long r = rbase + 64 * i; rl[i] = r < m_pad ? r : m_pad - 1; v[i] = 0.0; }
  const int nd = s0 < S ? (S - s0 < Sg ? S - s0 : Sg) : 0;     // digits of this group
  for (int d = nd - 1; d >= 0; d -= 2) {                        // smallest scale first, two digits per step (the lower one masked when d == 0)
    const int d1 = d > 0 ? d - 1 : 0;
    const int *pa = p0 + (size_t)(s0 + d) * nc * m_pad, *pb = p0 + (size_t)(s0 + d1) * nc * m_pad;
    long long ta[kFinTRows], tb[kFinTRows];
#pragma unroll
    for (int i = 0; i < kFinTRows; i++) { ta[i] = 0; tb[i] = 0; }
    for (int sp = 0; sp < splits; sp++) {
      const size_t off = (size_t)sp * e_pad * m_pad;
      int xa[kFinTRows], xb[kFinTRows];
#pragma unroll
      for (int i = 0; i < kFinTRows; i++) { xa[i] = pa[off + rl[i]]; xb[i] = pb[off + rl[i]]; }
#pragma unroll
      for (int i = 0; i < kFinTRows; i++) { ta[i] += xa[i]; tb[i] += xb[i]; }
    }
#pragma unroll
    for (int i = 0; i < kFinTRows; i++) {
      v[i] += ldexp((double)ta[i], Ej - 8 * (s0 + d + 1));
      if (d > 0) v[i] += ldexp((double)tb[i], Ej - 8 * (s0 + d1 + 1));
    }
  }
#pragma unroll
  for (int i = 0; i < kFinTRows; i++) part[g][64 * i + lane] = v[i];
  __syncthreads();
  // thread (lane, g) finishes row 64 g + lane of the block
  const long r = (long)blockIdx.x * kFinTBlockRows + threadIdx.x;
  if (r >= fill_rows) return;
  double out = 0.0;
  if (r < m) {
    if (bad) out = __longlong_as_double(0x7ff8000000000000ll);
    else out = ((part[3][threadIdx.x] + part[2][threadIdx.x]) + part[1][threadIdx.x]) + part[0][threadIdx.x];
    if (centered) {
      if (mode_trans) out = fma(-2.0 * sumB[j], f[r], out);
      else out += -2.0 * sumfB[j];
    }
  }
  Cout[r + (long)j * ldc] = out;
}

// n <= 2 (one tile of 32 expanded columns, e = s * nc + jj, nc * S <= 32, nc = 1 or 2).  Pure HBM streaming: splits x 128 bytes per row.  Eight
// threads share a row, each with four digits (one 16-byte load per split -- a wave reads 1 KiB runs); four rows per thread, all their loads
// issued before the first use.  A thread adds its digits' int32 partials of all K splits exactly (int64), scales them (exact) and adds its four
// terms smallest scale first; the eight threads of a row are then added in a fixed butterfly (3 levels): at most 6 roundings per result.
// (Round 2 read 4 bytes per lane: 2.7-3.3 TB/s; 35-47 us of a 1.1 ms product.)
constexpr int kFinSmallRows = 4;       // rows per thread
constexpr int kFinSmallBlockRows = 32 * kFinSmallRows;
__global__ void __launch_bounds__(256) k_finish_i8_small(const int *__restrict__ P, long m_pad, int splits, long m, int n, int S, int nc, const int *__restrict__ E,
                                                         const double *__restrict__ colmax_part, double *__restrict__ Cout, long ldc, long fill_rows, int mode_trans,
                                                         int centered, const double *__restrict__ sumB, const double *__restrict__ sumfB, const double *__restrict__ f,
                                                         const int *__restrict__ skip_if_set) {
  if (skip_if_set && *skip_if_set) return;
  const int g = threadIdx.x & 7;                                       // digits 4g .. 4g+3 of the row
  const long rbase = (long)blockIdx.x * kFinSmallBlockRows + (threadIdx.x >> 3);
  long long t[kFinSmallRows][4];
  long rl[kFinSmallRows];
#pragma unroll
  for (int i = 0; i < kFinSmallRows; i++) {
    const long r = rbase + 32 * i;
    rl[i] = r < m_pad ? r : m_pad - 1;                                 // clamped loads; rows >= m are masked below
#pragma unroll
    for (int d = 0; d < 4; d++) t[i][d] = 0;
  }
  const int4 *P4 = reinterpret_cast<const int4 *>(P);
  for (int sp = 0; sp < splits; sp++) {
    int4 x[kFinSmallRows];
#pragma unroll
    for (int i = 0; i < kFinSmallRows; i++) x[i] = P4[((size_t)sp * m_pad + rl[i]) * 8 + g];
#pragma unroll
    for (int i = 0; i < kFinSmallRows; i++) { t[i][0] += x[i].x; t[i][1] += x[i].y; t[i][2] += x[i].z; t[i][3] += x[i].w; }
  }
  // digit e = 4g + d belongs to column jj = e % nc, slice s = e / nc, weight 2^(E_jj - 8(s+1))
  int sh[4]; bool live[4];
#pragma unroll
  for (int d = 0; d < 4; d++) {
    const int e = 4 * g + d, sl = e / nc, jj = e - sl * nc;
    live[d] = e < nc * S;
    sh[d] = live[d] ? E[jj] - 8 * (sl + 1) : 0;
  }
  bool bad[2] = {false, false};
  double cs[2] = {0.0, 0.0};
  for (int jj = 0; jj < nc && jj < n; jj++) {
    double cm = 0.0;
    for (int c = 0; c < 64; c++) cm = fmax(cm, colmax_part[(size_t)jj * 64 + c]);
    bad[jj] = !(cm <= 1.7976931348623157e308);                        // a column with inf / NaN: NaN, like 0 * inf in fp64
    if (centered) cs[jj] = -2.0 * (mode_trans ? sumB[jj] : sumfB[jj]);
  }
#pragma unroll
  for (int i = 0; i < kFinSmallRows; i++) {
    const long r = rbase + 32 * i;
    double v[2] = {0.0, 0.0};
#pragma unroll
    for (int d = 3; d >= 0; d--) {                                     // smallest scale first
      const double term = (live[d] && r < m) ? ldexp((double)t[i][d], sh[d]) : 0.0;
      if (nc == 1) v[0] += term; else v[d & 1] += term;
    }
#pragma unroll
    for (int jj = 0; jj < 2; jj++)
      for (int off = 4; off >= 1; off >>= 1) v[jj] += __shfl_xor(v[jj], off, 8);
    if (g < nc && g < n && r < fill_rows) {
      double out = v[g];
      if (r < m) {
        if (bad[g]) out = __longlong_as_double(0x7ff8000000000000ll);
        if (centered) out = mode_trans ? fma(cs[g], f[r], out) : out + cs[g];
      } else out = 0.0;
      Cout[r + (long)g * ldc] = out;
    }
  }
}

// (the plan of a product -- I8Plan, plan_i8, the split table, the choice of finish: mxa_plan.h, host-only code swept on the CPU)
template <int NT, int MT, int WC, bool SWAP1 = false>
static int launch_i8_t(const PackedMatrix &G, const int8_t *dBs, int *dP, const I8Plan &p, hipStream_t s, const int *skip_if_set, const I8Direct &dir) {
  using Cfg = I8Cfg<NT>;
  static unsigned long long attr_a = 0;   // function attributes are per device
  if (ensure_dyn_lds(reinterpret_cast<const void *>(&k_gemm_i8<NT, MT, WC, SWAP1>), Cfg::kLds, &attr_a)) return 1;
  const long grid = (long)p.rowblocks * p.nchunks * p.splits;
  hipLaunchKernelGGL((k_gemm_i8<NT, MT, WC, SWAP1>), dim3((unsigned)grid), dim3(256), Cfg::kLds, s, G.d, G.pitch, dBs, p.T_total, dP, p.m_pad, p.e_pad,
                     p.rowblocks, p.nchunks, p.stages_total, make_split_tab(p.stages_total, p.splits, kPlanI8MaxSplitStages), (unsigned long long *)nullptr, skip_if_set, dir);
  MXA_HIP(hipGetLastError());
  return 0;
}

// Whole product on the device; B, C device pointers; asynchronous on s.  The workspace (exponents, slices, partials) lives with the
// handle and only grows.
// K splits of the transposed-operand kernel: workgroups = strips x splits on one resident workgroup per CU; the split count whose last round of
// workgroups is fullest, counting a start-up worth a few stages per workgroup; at most 2047 stages per split (int32 accumulators)
constexpr int kTnBufs = 4;   // 4 buffers x 2 workgroups per CU: 3 stages in flight.  (3 x 3 needs <= 168 VGPRs; the kernel holds 206, 128 of them accumulators: forcing the bound makes the
                             // compiler spill 34 dwords inside the stage loop -- round 6 -- and scratch traffic shares the vmcnt the hand-written waits count: not an option without a smaller wave tile)
// Items of the transposed-operand kernel: the first n_lo strips are cut into c_lo equal pieces of their K range, the other strips into c_lo + 1; the items of
// the c_lo-piece strips (the longer ones) come first, piece-major.  Chosen so that the items fill whole rounds of the resident slots with (nearly) equal
// lengths inside every round: cost = sum over the rounds of (longest item of the round + a few stages of start-up and flush), fewest pieces among equals.
static TnSched plan_i8_tn(long indiv_slabs, long snp_rows, int tiles_per_pass) {
  static const long cus = [] {
    int dev = 0; hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess || prop.multiProcessorCount <= 0) { (void)hipGetLastError(); return 256L; }
    return (long)prop.multiProcessorCount;
  }();
  const char *e = getenv("MXA_TN_SCHED");                                  // A/B runs and tests: 0 / 1 = the mode, if the shape allows it (read per product:
  const int force = e && *e ? atoi(e) : -1;                                // tools/ab_env.py alternates the two inside one process, on one clock)
  return plan_i8_tn_host(indiv_slabs, snp_rows, cus * (tiles_per_pass == 1 ? 2 : 1), tiles_per_pass, force);
}

template <int BUFS, int TT>
static int launch_i8_tn(const PackedMatrix &G_tn, const int8_t *d_Bs, int *d_P, const I8Plan &p, const TnSched &sc, hipStream_t s, const int *skip) {
  static unsigned long long attr_tn = 0;
  if (ensure_dyn_lds(reinterpret_cast<const void *>(&k_gemm_i8_tn<BUFS, TT>), (TnCfg<BUFS, TT>::kLds), &attr_tn)) return 1;
  const unsigned grid = (unsigned)tn_grid(sc);   // persistent: one workgroup per resident slot (mode 0: fewer if there are fewer items)
  constexpr int lds = TnCfg<BUFS, TT>::kLds;
  for (int nt = 0; nt < p.NT; nt += TT)
    hipLaunchKernelGGL((k_gemm_i8_tn<BUFS, TT>), dim3(grid), dim3(256), lds, s, G_tn.d, G_tn.nslabs, d_Bs + (size_t)nt * 1024, p.NT, d_P, p.m_pad, p.e_pad,
                       nt * 32, sc, skip);
  MXA_HIP(hipGetLastError());
  return 0;
}

// plan of one product (plain or transposed-operand form) and the bytes of workspace it needs; returns 2 when the transposed form declines
struct I8Full { I8Plan p; bool tn; int tn_strips, tn_stages; TnSched tn_sc; size_t part_bytes, e_bytes, bs_bytes, p_bytes, need; };
static int plan_i8_full(const PackedMatrix &G, int n, int S_override, const PackedMatrix *G_tn, I8Full &f) {
  const long m = G.rows, k = G.k;
  f.p = plan_i8(m, G.k_pad, n, S_override);
  I8Plan &p = f.p;
  if (p.m_pad > G.rows_pad) { set_error(4, "internal: packed matrix smaller than the i8 plan"); return 1; }
  if (p.splits > kMaxI8Splits) { set_error(4, "int8 engine: K of %ld genotypes needs more than %d K splits", G.k_pad, kMaxI8Splits); return 1; }   // beyond 64 x 32767 stages: the split table ends there
  // transposed-operand form (G_tn = the copy whose ROWS are the K index): same digits, same exactness guard, other main kernel and P layout
  // (several tiles of 32 expanded columns: one pass over the matrix per tile -- 3 <= n <= 6 and peeled columns of single-orientation objects; beyond what the
  // fp64 MFMA tile would take, or with several column chunks, the caller's fp64 path is the better choice: declined with 2 before anything is enqueued)
  // round 5: tiles are taken two per pass (k_gemm_i8_tn<.., 2>); more than three passes cost more than the fp64 path
  if (G_tn != nullptr && (p.nchunks != 1 || (p.NT + 1) / 2 > 3)) return 2;
  if (G_tn != nullptr && p.NT >= 2 && (p.NT & 1)) { p.NT += 1; p.e_pad = p.nchunks * p.NT * 32; }   // an even number of tiles: the last pass multiplies a tile of zero digits (the launch is bound by the packed stream)
  f.tn = G_tn != nullptr;
  // host-side operand check before anything is enqueued: a kernel must never be handed the dimensions-only descriptor of a copy that is not stored
  if ((f.tn ? G_tn->d : G.d) == nullptr) { set_error(4, "internal: the int8 route was given a packed matrix that is not stored (single-orientation object)"); return 1; }
  f.tn_strips = f.tn_stages = 0; f.tn_sc = TnSched{};
  if (f.tn) {
    if (G_tn->k != m || G_tn->rows != k) { set_error(4, "internal: transposed operand has the wrong shape"); return 1; }
    f.tn_sc = plan_i8_tn(G_tn->nslabs, G_tn->rows, p.NT >= 2 ? 2 : 1);
    f.tn_strips = f.tn_sc.strips; f.tn_stages = f.tn_sc.K;
    if ((long)f.tn_stages * kTileRows > G_tn->rows_pad) { set_error(4, "internal: packed matrix smaller than the transposed i8 plan"); return 1; }
    if (f.tn_sc.mode == 0 && (f.tn_stages + f.tn_sc.q1 - 1) / f.tn_sc.q1 > kTnMaxPieceStages) return 2;   // K beyond 64 x 2047 row blocks (33.5 M SNPs in one object): the fp64 path
    // splits = partial-sum slots per strip
    p.T_total = (long)f.tn_stages * 8; p.splits = f.tn_sc.pslots; p.m_pad = (long)f.tn_strips * kTnSlabs * kSlabK; p.e_pad = p.NT * 32;
  }
  auto up = [](size_t x) { return (x + 255) / 256 * 256; };
  f.part_bytes = up(sizeof(double) * 128 * n); f.e_bytes = up(sizeof(int) * (n + 1));   // column maxima + minima; exponents
  f.bs_bytes = up((size_t)p.nchunks * p.T_total * p.NT * 1024);
  f.p_bytes = up(sizeof(int) * (size_t)p.splits * p.m_pad * p.e_pad);
  f.need = f.part_bytes + f.e_bytes + f.bs_bytes + f.p_bytes;
  return 0;
}
static int i8_grow(Workspace &w, size_t need, hipStream_t s) {
  if (w.cap_i8 >= need) return 0;
  MXA_HIP(hipStreamSynchronize(s));
  if (w.d_i8) { MXA_HIP(hipFree(w.d_i8)); w.d_i8 = nullptr; w.cap_i8 = 0; }
  MXA_HIP(hipMalloc(&w.d_i8, need));
  w.cap_i8 = need;
  return 0;
}
// room for the chains of a guarded product BEFORE the first one is enqueued (growing the workspace waits for the stream: once per object and shape)
int gemm_i8_reserve(const PackedMatrix &G, int n, int S, const PackedMatrix *G_tn, Workspace &w, hipStream_t s) {
  I8Full f;
  const int rc = plan_i8_full(G, n, S, G_tn, f);
  if (rc) return rc;
  return i8_grow(w, f.need, s);
}

int gemm_i8_device(const PackedMatrix &G, bool trans, int n, const double *dB, long ldb, double *dC, long ldc, long fill_rows, bool centered, double *d_sumB,
                   double *d_sumfB, const double *d_f, Workspace &w, hipStream_t s, const I8Opts &o) {
  hipEvent_t ev0 = o.ev0, ev1 = o.ev1;
  int *splits_out = o.splits_out, S_override = o.S_override;
  const int **flag_out = o.flag_out;
  double *colsum_scratch = o.colsum_scratch, *stats_part = o.stats_part;
  const PackedMatrix *G_tn = o.G_tn; const I8Chain *chain = o.chain;
  const long m = G.rows, k = G.k;
  if (chain) {   // guarded product, device-side verdict: this launch sequence is the chain of one class
    if (n > kSmallNMaxCols || !colsum_scratch) { set_error(4, "internal: guarded int8 chain with %d columns", n); return 1; }
    S_override = chain->my_class ? chain->S1 : chain->S0;
  }
  I8Full pf;
  {
    const int rcp = plan_i8_full(G, n, S_override, G_tn, pf);
    if (rcp) return rcp;
  }
  I8Plan &p = pf.p;
  const bool tn = pf.tn;
  if (splits_out) *splits_out = p.splits;
  const size_t part_bytes = pf.part_bytes, e_bytes = pf.e_bytes, bs_bytes = pf.bs_bytes;
  if (chain && !chain->first && w.cap_i8 < pf.need) { set_error(4, "internal: the second chain of a guarded product outgrows the workspace (gemm_i8_reserve)"); return 1; }
  if (i8_grow(w, pf.need, s)) return 1;
  char *base = static_cast<char *>(w.d_i8);
  double *d_part = (stats_part && !chain) ? stats_part : reinterpret_cast<double *>(base);
  int *d_E = reinterpret_cast<int *>(base + part_bytes);
  int8_t *d_Bs = reinterpret_cast<int8_t *>(base + part_bytes + e_bytes);
  int *d_P = reinterpret_cast<int *>(base + part_bytes + e_bytes + bs_bytes);

  // E_j = e + 2: |b| * 2^-E_j < 1/4, inside the remainder range of the balanced digits
  const int *skip = nullptr;   // a chain: the kernels below test this device flag themselves
  SliceFused fu{};
  if (!chain) {
    if (stats_part) { if (launch_colexp_from_part(d_part, n, d_E, 2, s)) return 1; }
    else if (launch_colexp(dB, ldb, k, n, d_part, d_E, 2, s)) return 1;
  } else {
    // Exactness guard of the default small-n route.  With |b| = f 2^e, f in [1/2, 1), an entry is the integer m 2^(e-53);
    // the last digit has weight 2^(E_j - 8S) = 2^(e_max + 2 - 8S).  Every entry is an exact multiple of it iff e_min - 53 >= e_max + 2 - 8S,
    // i.e. the exponent span e_max - e_min <= 8S - 55; the recombination ldexp(t, E_j - 8(s+1)) stays normal iff e_max + 2 - 8S >= -1021.
    // the flag lives in the handle's small flag block (never reallocated while the handle lives: mxa_last_path() may read it later)
    if (!w.d_denflag) { set_error(4, "internal: flag block missing"); return 1; }
    int *d_flag = w.d_denflag + 1;   // three words: (class == 2), (class != 0), (class != 1)   [SliceFused]
    // one statistics pass (the first chain's); exponents, verdict and column sums are finished inside k_slice_B
    if (chain->first) hipLaunchKernelGGL(k_colstats_partial, dim3(64, n), dim3(256), 0, s, dB, ldb, k, n, trans ? nullptr : d_f, centered ? 1 : 0, d_part, colsum_scratch);
    fu = SliceFused{d_part, colsum_scratch, d_E, d_flag, d_sumB, d_sumfB, 2, chain->S0, chain->S1, chain->my_class, chain->first ? 1 : 0, centered ? 1 : 0};
    skip = d_flag + 1 + chain->my_class;     // (class != my_class)
    if (flag_out) *flag_out = d_flag;        // (class == 2): the fp64 kernel behind runs iff it is set
  }
  if (p.NT * 32 != p.nc * p.S) MXA_HIP(hipMemsetAsync(d_Bs, 0, bs_bytes, s));   // expanded columns beyond nc*S are never written
  {
    const int ncols = p.nchunks * p.nc;
    const long total = (long)p.T_total * 2 * ncols * 4;
    SmallNFallback fb{};
    long blocks = (total + 255) / 256;
    if (chain && chain->first && chain->fp64_rows) {   // the fp64 rows of verdict class 2 ride in this launch: a thread per output row (n = 1; wider chains: gated fp64 launches of the caller)
      const PackedMatrix &GF = tn ? *G_tn : G;
      fb = SmallNFallback{GF.d, GF.nslabs, m, k, dC, ldc, fill_rows, tn ? 1 : 0, trans ? 1 : 0, centered ? 1 : 0, d_f};
      blocks = std::max(blocks, (fill_rows + 255) / 256);
    }
    hipLaunchKernelGGL(k_slice_B, dim3((unsigned)std::min<long>(blocks, 256L * 64)), dim3(256), 0, s, dB, ldb, k, n, d_E, p.S, p.nc, p.NT,
                       p.T_total, ncols, reinterpret_cast<uint32_t *>(d_Bs), total, skip, fu, tn ? 1 : 0, fb);
  }
  MXA_HIP(hipGetLastError());
  if (ev0) MXA_HIP(hipEventRecord(ev0, s));
  int rc = 0;
  I8Direct dir{};
  if (tn) {
    if (p.NT >= 2 ? launch_i8_tn<6, 2>(*G_tn, d_Bs, d_P, p, pf.tn_sc, s, skip)
                  : launch_i8_tn<kTnBufs, 1>(*G_tn, d_Bs, d_P, p, pf.tn_sc, s, skip)) return 1;
    if (ev1) MXA_HIP(hipEventRecord(ev1, s));
    static_assert(kFinTBlockRows == kTnSlabs * kSlabK, "a block of k_finish_i8_t = one strip of k_gemm_i8_tn: it adds that strip's slots");
    dim3 grid((unsigned)((fill_rows + kFinTBlockRows - 1) / kFinTBlockRows), (unsigned)n);
    hipLaunchKernelGGL(k_finish_i8_t, grid, dim3(256), 0, s, d_P, p.m_pad, p.e_pad, p.splits, m, n, p.S, p.nc, p.NT, d_E, d_part, dC, ldc, fill_rows, trans ? 1 : 0,
                       centered ? 1 : 0, d_sumB, d_sumfB, d_f, skip, 1, pf.tn_sc);
    MXA_HIP(hipGetLastError());
    return chain ? 3 : 0;
  }
  const I8Finish finish = i8_finish_route(p);
  if (finish == I8Finish::direct)
    dir = I8Direct{1, d_E, d_part, dC, ldc, m, fill_rows, n, p.S, p.nc, trans ? 1 : 0, centered ? 1 : 0, d_sumB, d_sumfB, d_f};
  switch (p.NT) {
    // one tile, three or more columns (n = 3; n = 4 with few digits): transposed partial sums like the wider launches (k_finish_i8_t)
    case 1: rc = finish == I8Finish::transposed ? launch_i8_t<1, 2, 1, true>(G, d_Bs, d_P, p, s, skip, dir) : launch_i8_t<1, 2, 1>(G, d_Bs, d_P, p, s, skip, dir); break;
    case 2: rc = launch_i8_t<2, 2, 1>(G, d_Bs, d_P, p, s, skip, dir); break;
    case 3: rc = launch_i8_t<3, 2, 1>(G, d_Bs, d_P, p, s, skip, dir); break;
    case 4: rc = launch_i8_t<4, 2, 1>(G, d_Bs, d_P, p, s, skip, dir); break;
    case 5: rc = launch_i8_t<5, 2, 1>(G, d_Bs, d_P, p, s, skip, dir); break;
    case 6: rc = launch_i8_t<6, 2, 1>(G, d_Bs, d_P, p, s, skip, dir); break;
    case 7: rc = launch_i8_t<7, 2, 1>(G, d_Bs, d_P, p, s, skip, dir); break;
    default: rc = launch_i8_t<8, 4, 2>(G, d_Bs, d_P, p, s, skip, dir); break;
  }
  if (rc) return rc;
  if (ev1) MXA_HIP(hipEventRecord(ev1, s));
  switch (finish) {
    case I8Finish::direct: break;   // finished inside k_gemm_i8
    case I8Finish::small:           // n <= 2: one tile, the fast finish
      hipLaunchKernelGGL(k_finish_i8_small, dim3((unsigned)((fill_rows + kFinSmallBlockRows - 1) / kFinSmallBlockRows)), dim3(256), 0, s, d_P, p.m_pad, p.splits, m, n, p.S, p.nc, d_E, d_part, dC, ldc, fill_rows,
                         trans ? 1 : 0, centered ? 1 : 0, d_sumB, d_sumfB, d_f, skip);
      break;
    case I8Finish::transposed: {    // operand-swapped instantiations: transposed partial sums
      dim3 grid((unsigned)((fill_rows + kFinTBlockRows - 1) / kFinTBlockRows), (unsigned)n);
      hipLaunchKernelGGL(k_finish_i8_t, grid, dim3(256), 0, s, d_P, p.m_pad, p.e_pad, p.splits, m, n, p.S, p.nc, p.NT, d_E, d_part, dC, ldc, fill_rows, trans ? 1 : 0,
                         centered ? 1 : 0, d_sumB, d_sumfB, d_f, skip, 0, TnSched{});
      break;
    }
  }
  MXA_HIP(hipGetLastError());
  return chain ? 3 : 0;
}

}  // namespace mxa
