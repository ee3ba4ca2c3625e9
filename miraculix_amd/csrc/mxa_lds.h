// mxa_lds.h -- the LDS-DMA and 2-bit unpack primitives shared by the MFMA kernels (mxa_kernels.hip: k_gemm, k_lut; mxa_gemm_i8.hip: k_gemm_i8, k_gemm_i8_tn;
// mxa_crossprod.hip: the crossproduct kernels).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mxa {

typedef int v4i __attribute__((ext_vector_type(4)));
using lptr_t = __attribute__((address_space(3))) void *;

// LDS-DMA with a wave-uniform 64-bit base in SGPRs, a per-lane 32-bit byte offset and a wave-uniform LDS byte address
// (M0).  Written as asm so that the per-slab address arithmetic stays on the scalar unit; hipcc does not count this
// load: a kernel waits for it with its own s_waitcnt vmcnt before the barrier that precedes the first ds_read of the data.
__device__ __forceinline__ void dma16_s(const void *sbase, uint32_t voff, uint32_t lds_addr) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %0" ::"s"(sbase), "v"(voff), "s"(lds_addr) : "memory", "m0");
}
// The same with the NON-TEMPORAL hint (NT), for the packed genotype tiles: they are read once per pass and are far larger than the L2s and the Infinity
// Cache, so letting them allocate there only costs bandwidth.  tools/hbm_read_probe.hip on MI355X: an LDS-DMA stream reads 6.9-7.0 TB/s with `nt`
// against 6.4-6.5 without (plain 16-byte loads: 7.1 against 6.3).  Operands that every row block re-reads (digit slabs, B fragments) keep the default policy.
// Measured on the config-5 shard (profiles/r03_nt_stream_ab.txt): k_gemm_i8 at n = 1 0.96-0.97 ms with the hint against 1.01-1.02 without; the lookup kernel
// k_lut 1.66 against 1.63 (LDS-bound: no gain, MXA_NT_LUT stays 0).  k_gemm is MFMA-bound and its time does not move (C2: 43.89-43.99 ms with, 43.87-44.02
// without), but its HBM traffic does: the packed stream no longer pushes the B-fragment slabs, which every row block re-reads, out of the L2s --
// 15.0 GB per launch by the counters instead of 18.9 (12.8 algorithmic; FETCH_SIZE calibrated for the hinted stream too: factor 2.000,
// profiles/r03_pmc_calibration_nt.json).  The units choose with their A/B macros: MXA_NT_GEMM = 1, MXA_NT_LUT = 0, MXA_NT_STREAM = 1.
template <bool NT>
__device__ __forceinline__ void dma16_p(const void *sbase, uint32_t voff, uint32_t lds_addr) {
  if (NT) asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %0 nt" ::"s"(sbase), "v"(voff), "s"(lds_addr) : "memory", "m0");
  else dma16_s(sbase, voff, lds_addr);
}

// 16 two-bit fields of a dword -> 16 int8 in 4 dwords: field 4i + q goes to byte i of register q (the int8 kernels permute the field order identically for
// both operands, or arrange the other operand to match: k_slice_B)
__device__ __forceinline__ v4i unpack16(uint32_t w) {
  v4i r;
  r[0] = (int)(w & 0x03030303u);
  r[1] = (int)((w >> 2) & 0x03030303u);
  r[2] = (int)((w >> 4) & 0x03030303u);
  r[3] = (int)((w >> 6) & 0x03030303u);
  return r;
}

}  // namespace mxa
