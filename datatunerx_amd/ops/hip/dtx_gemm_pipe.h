// The byte-level pipeline pieces of the 256x256 MFMA GEMMs (gemm.hip bf16,
// gemm_fp8.hip e4m3): buffer resource descriptors, the LDS-DMA load, the
// counted waits, the raw barrier and the half-slot swizzle. None of them
// knows an element type: a half-slot is [256 rows][64 B] for both kernels.
#pragma once

#include "dtx_mfma.h"

typedef __attribute__((ext_vector_type(4))) unsigned uint4v;
typedef __attribute__((ext_vector_type(2))) unsigned uint2v;

// Buffer resource descriptor (T8/T20): built from readfirstlane'd scalars
// so hipcc proves uniformity (no waterfall loops), num_records = bytes so
// out-of-bounds rows of the M-tail clamp to zero loads / dropped stores.
__device__ __forceinline__ uint4v dtx_srd(const void* base,
                                          unsigned long long bytes) {
  unsigned long long b = (unsigned long long)base;
  uint4v r;
  r.x = __builtin_amdgcn_readfirstlane((unsigned)b);
  r.y = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
  r.z = __builtin_amdgcn_readfirstlane((unsigned)bytes);
  r.w = 0x00020000u;  // dfmt/nfmt raw buffer config
  return r;
}

// LDS-DMA: stage 64 lanes x 16 B at global (srd + voff) into LDS at
// wave-uniform byte base `lds_dst` + lane*16. M0 written in the same
// statement (s_nop 0 = the required wait state after the M0 write).
__device__ __forceinline__ void glds16(uint4v srd, unsigned voff,
                                       unsigned lds_dst) {
  asm volatile(
      "s_mov_b32 m0, %1\n\t"
      "s_nop 0\n\t"
      "buffer_load_dwordx4 %0, %2, 0 offen lds"
      :: "v"(voff), "s"(lds_dst), "s"(srd) : "memory");
}

__device__ __forceinline__ void dtx_vmcnt8() {
  asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
}
__device__ __forceinline__ void dtx_vmcnt7() {
  asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
}
__device__ __forceinline__ void dtx_vmcnt0() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
__device__ __forceinline__ void dtx_bar() {
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

#define GEMM_BM 256
#define GEMM_BN 256
#define HALF_BYTES (256 * 64)          // one [256 rows][64 B] half-slot

// f((r>>2)&3) of the swizzle: 0->0, 1->3, 2->2, 3->1  == (-x)&3
__device__ __forceinline__ unsigned swz_f(unsigned x) { return (0u - x) & 3u; }

// Block -> (mb, nb) of the 256x256 tile grid, nbn = N / 256 column blocks.
// GRID: 1 = 8mb x 4nb clusters inside each XCD chunk of the remapped
//       block order (A-panel reuse in L2/L3 as well as B; needs
//       mb_n % 8 == 0 and nb_n % 4 == 0); 2 = 8-row mb-groups sweeping
//       all nb in dispatch order (general shapes, L3-bounded window;
//       the last group may hold fewer than 8 rows).
template <int GRID>
__device__ __forceinline__ void dtx_gemm_block(int nbn, int mb_n, int& mb,
                                               int& nb) {
  static_assert(GRID == 1 || GRID == 2, "GRID: 1 = clusters, 2 = snake");
  if (GRID == 1) {
    // XCD-aware bijective remap, then 32-block clusters of 8(mb) x
    // 4(nb); clusters enumerated nb-major
    const int nwg = gridDim.x;
    const int q = nwg >> 3, r8 = nwg & 7;
    const int xcd = blockIdx.x & 7, pos = blockIdx.x >> 3;
    const int wgid =
        (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + pos;
    const int mbc = mb_n >> 3;
    const int cl = wgid >> 5, ci = wgid & 31;
    mb = (cl % mbc) * 8 + (ci & 7);
    nb = (cl / mbc) * 4 + (ci >> 3);
  } else {
    // 8-row mb-groups sweeping ALL nb columns, dispatch order (no XCD
    // remap): the ~256 concurrently-resident blocks then span <= 2
    // groups, so the A-panel (16 rows x K) and B re-reads stay
    // L3-resident chip-wide instead of streaming A from HBM once per
    // nb column (PMC: FETCH dropped ~4x on the mb24 shapes).
    const int g = blockIdx.x / (nbn * 8);
    const int rem = blockIdx.x % (nbn * 8);
    const int rows = min(8, mb_n - g * 8);
    nb = rem / rows;
    mb = g * 8 + rem % rows;
  }
}
