// mxa_ldop_host.h -- the host-only part of the LD operator object (mxa_ldop.hip): the check of `last`, the layout arrays and the byte count.
// Plain C++ without any HIP header, so that a stand-alone program can compile it for the CPU (tools/ldop_host_check.cpp, run under
// -fsanitize=address,undefined).
#pragma once
#include <cstddef>

namespace mxa {

// the window is data: i <= last[i] < snps, non-decreasing.  Returns -1 when it holds, else the first index that breaks it.
inline long ldop_check_last(long snps, const int *last) {
  for (long i = 0; i < snps; i++) {
    const long l = last[i];
    if (l < i || l >= snps || (i > 0 && l < last[i - 1])) return i;
  }
  return -1;
}

// The layout of a checked window.  first[i] = min{k : last[k] >= i} (a two-pointer sweep: first never moves back); rowptr = exclusive prefix sum of
// last[i] - i + 1 (the upper ragged rows of mxa_ld_window_rows); ptr = exclusive prefix sum of last[i] - first[i] + 1 (the mirrored rows).  first: snps
// ints, rowptr and ptr: snps + 1 longs; each may be nullptr.  Returns the number of upper entries, rowptr[snps]; *mirrored = ptr[snps] = 2 entries - snps.
inline long ldop_layout(long snps, const int *last, int *first, long *rowptr, long *ptr, long *mirrored) {
  long up = 0, full = 0, k = 0;
  if (rowptr) rowptr[0] = 0;
  if (ptr) ptr[0] = 0;
  for (long i = 0; i < snps; i++) {
    while (last[k] < i) k++;           // last[i] >= i: k <= i, the sweep ends
    if (first) first[i] = (int)k;
    up += (long)last[i] - i + 1;
    full += (long)last[i] - k + 1;
    if (rowptr) rowptr[i + 1] = up;
    if (ptr) ptr[i + 1] = full;
  }
  if (mirrored) *mirrored = full;
  return up;
}

// device bytes an object holds after creation: the mirrored rows, first and last (ints), ptr and rowptr (snps + 1 longs each), base (snps longs) and the
// packed column chunk of an apply (16 doubles per SNP)
inline long ldop_object_bytes(long snps, long mirrored) {
  return (long)sizeof(double) * mirrored + 2 * (long)sizeof(int) * snps + 2 * (long)sizeof(long) * (snps + 1) + (long)sizeof(long) * snps +
         16 * (long)sizeof(double) * snps;
}

}  // namespace mxa
