// NF4 (NormalFloat4) codebook shared by the bulk dequant (quant.hip) and
// the weight-streaming decode kernels (qgemv_nf4.hip). Format of
// models/quant.py: packed [N,K/2] uint8, low nibble = even k, nibble =
// index into the 16 levels below; absmax [N,K/group] f32; weight =
// level[index] * absmax.
#pragma once

#include "dtx_common.h"

// the 16 published fp32 levels (QLoRA), monotone, index 7 = 0
__device__ __forceinline__ float dtx_nf4_level(int i) {
  constexpr float code[16] = {
      -1.0f, -0.6961928009986877f, -0.5250730514526367f,
      -0.39491748809814453f, -0.28444138169288635f, -0.18477343022823334f,
      -0.09105003625154495f, 0.0f, 0.07958029955625534f,
      0.16093020141124725f, 0.24611230194568634f, 0.33791524171829224f,
      0.44070982933044434f, 0.5626170039176941f, 0.7229568362236023f,
      1.0f};
  return code[i & 15];
}
