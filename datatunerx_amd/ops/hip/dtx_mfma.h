// MFMA helpers shared by the matrix-core kernels (gemm, attn_fwd,
// attn_bwd, lora, qgemv): intrinsic wrappers, fragment vector types,
// softmax constants and the 32x32 C-layout <-> fragment conversions.
#pragma once

#include "dtx_common.h"

// a, b: short8v (8 bf16 per lane); c: f32x4 (16x16) / f32x16 (32x32).
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0)
#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)

typedef float4v f32x4;
typedef float16v f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

#define NEG_INF (-3.0e38f)
#define LOG2E 1.4426950408889634f
#define LN2 0.6931471805599453f

#define DTX_AS3 __attribute__((address_space(3)))

// C-layout row index for f32x16 accumulator register r (32x32 MFMA);
// the column is lane & 31, hi = lane >> 5.
__device__ __forceinline__ int crow(int r, int hi) {
  return (r & 3) + 8 * (r >> 2) + 4 * hi;
}

// MFMA B-fragment gathered from a ROW-major [k][n] LDS image with
// ds_read_b64_tr_b16 (gfx950 hardware 4x4 transpose read) — replaces
// a separately-staged transposed image. Verified mapping
// (tools/probe_tr.cpp): with 16-lane-group addresses
// R_i = &img[k0 + (i>>2)][n0 + 4*(i&3)], lane l = 4a+c receives
// component j = img[k0 + j][n0 + (l&15)] — exactly B[k][n=l&31] when
// n0 = 32-col base + 16*((l>>4)&1). Two reads cover the lane's 8 ks.
// img must be an address_space(3) pointer so all address math stays in
// 32-bit LDS offsets (a generic pointer here costs 64-bit address
// arithmetic per read and ~+120 VGPRs in the dkdv kernel).
template <int STRIDE>
__device__ __forceinline__ short8v tr_bfrag(
    const DTX_AS3 unsigned short* img, int k0, int n0, int lane) {
  const int row = k0 + ((lane >> 2) & 3);
  const int col = n0 + ((lane >> 4) & 1) * 16 + (lane & 3) * 4;
  const DTX_AS3 unsigned short* p = img + row * STRIDE + col;
  union { bf16x4 v[2]; short8v s; } u;
  u.v[0] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (DTX_AS3 bf16x4*)p);
  u.v[1] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (DTX_AS3 bf16x4*)(p + 4 * STRIDE));
  return u.s;
}

// C-layout f32x16 (rows R on regs, cols on lanes) -> two bf16 A/B
// fragments with k = R (frag0: R 0..15, frag1: R 16..31): 8 cvt_pk +
// 4 permlane32_swap, no LDS round trip.
__device__ __forceinline__ void conv_c_to_frag(const f32x16& p,
                                               short8v& f0, short8v& f1) {
  unsigned c0 = dtx_cvt_pk_bf16(p[0], p[1]);
  unsigned c1 = dtx_cvt_pk_bf16(p[2], p[3]);
  unsigned c2 = dtx_cvt_pk_bf16(p[4], p[5]);
  unsigned c3 = dtx_cvt_pk_bf16(p[6], p[7]);
  unsigned c4 = dtx_cvt_pk_bf16(p[8], p[9]);
  unsigned c5 = dtx_cvt_pk_bf16(p[10], p[11]);
  unsigned c6 = dtx_cvt_pk_bf16(p[12], p[13]);
  unsigned c7 = dtx_cvt_pk_bf16(p[14], p[15]);
  auto r02 = __builtin_amdgcn_permlane32_swap(c0, c2, false, false);
  auto r13 = __builtin_amdgcn_permlane32_swap(c1, c3, false, false);
  auto r46 = __builtin_amdgcn_permlane32_swap(c4, c6, false, false);
  auto r57 = __builtin_amdgcn_permlane32_swap(c5, c7, false, false);
  u32x4 lo{(unsigned)r02[0], (unsigned)r13[0],
           (unsigned)r02[1], (unsigned)r13[1]};
  u32x4 hi4{(unsigned)r46[0], (unsigned)r57[0],
            (unsigned)r46[1], (unsigned)r57[1]};
  f0 = *reinterpret_cast<short8v*>(&lo);
  f1 = *reinterpret_cast<short8v*>(&hi4);
}
