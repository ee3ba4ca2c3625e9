// mxa_ldprune.hip -- LD pruning and clumping (mxa_ld_prune_csr, mxa_ld_window_prune, mxa_ld_window_prune_pairwise): the greedy selection on the
// pairs graph, on the device.  The window entries take their graph from the pairs driver of mxa_ldwindow.hip (ld_pairs_any).
#include "../../include/miraculix_amd.h"
#include "mxa_xprod.h"
#include <algorithm>

namespace mxa {

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
