// Weight-streaming decode kernels for quantized base weights (gfx950):
//   y[M,N] = x[M,K] @ dequant(Wq)[N,K]^T, x/y bf16, fp32 accumulate,
// M <= 16. The integer weight is streamed once with 16-byte loads and
// dequantized in registers — no bf16 weight is ever written to HBM
// (the dequant-then-linear path moves >= 4.5 bytes per weight; this
// moves 1 or 0.5). Weight formats are models/quant.py's:
//   int8: q[N,K] int8, scale[N] f32 (per-row absmax)
//   int4: packed[N,K/2] uint8, low nibble = even k, stored value q+8,
//         scale[N,K/group] f32
//
// (a) M == 1: VALU streaming kernel in the shape of gemv.hip — a wave
//     owns RPW output rows, lanes take one 16-byte piece of each row per
//     step (16 int8 / 32 int4 weights), x is re-read from L1/L2, no LDS.
//     int8 applies the row scale once after the wave reduction; int4
//     scales each lane's 32-nibble partial sum (one group: group % 32
//     == 0) in fp32, and forms that sum with bf16 dot2 on nibbles turned
//     into bf16 by integer ops (the fp32 convert-and-fma form is
//     VALU/occupancy-bound at about the int8 kernel's weights/s). RPW
//     is chosen from N so a small N (a GQA k/v projection) still fills
//     the machine.
// (b) 2 <= M <= 16: MFMA kernel. The 16 weight rows of a tile are the A
//     operand of mfma_f32_16x16x32_bf16, the batch rows (zero-padded to
//     16 in registers) the B operand. The contraction is permuted: lane
//     (row r, quad h) takes the contiguous 16-byte piece h of the
//     step's weight row r and the matching contiguous piece of x row r,
//     so both operands use the same k mapping and every global load is
//     one contiguous 16 B. A block's waves split K (interleaved steps)
//     and share T 16-row tiles per x fragment; the partial accumulators
//     meet in LDS (no workspace, no memset: hipGraph-capturable).
//     Both widths feed exact integers as bf16 (int8: q; int4: 128 + nib,
//     the bias removed with the group's sum of x) and scale in fp32:
//     int8 scales the finished row sum, int4 gives every scale group of
//     a step a fresh accumulator and adds it scaled per weight row — so
//     M = 1 and M > 1 differ only in fp32 summation order (a batched
//     decode step reproduces the single-stream logits).
//
// Tails: rows past N-1 alias onto a valid row for loads and are never
// stored; lanes past K load nothing and feed zeros in BOTH operands;
// batch rows >= M are zeros in registers. Row offsets are long.
#include "dtx_mfma.h"
#include "dtx_launch.h"

typedef __attribute__((ext_vector_type(4))) unsigned uint4q;

typedef __attribute__((ext_vector_type(2))) float qg_f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 qg_bf16x2;

// two floats -> packed bf16 pair (RNE, one v_cvt_pk_bf16_f32), lo in
// bits 0..15
__device__ __forceinline__ unsigned qg_pack_bf16(float lo, float hi) {
  const qg_f32x2 f = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f, qg_bf16x2));
}

// c + a.lo*b.lo + a.hi*b.hi on packed bf16 pairs (v_dot2c_f32_bf16)
__device__ __forceinline__ float qg_dot2(unsigned a, unsigned b, float c) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(qg_bf16x2, a),
                                         __builtin_bit_cast(qg_bf16x2, b),
                                         c, false);
}

// sign-extended byte b of a dword
__device__ __forceinline__ float qg_sbyte(unsigned p, int b) {
  return (float)((int)(p << (24 - 8 * b)) >> 24);
}

// ------------------------------------------------------------ (a) M = 1
template <int BITS, int RPW>
__global__ __launch_bounds__(DTX_BLOCK)
void qgemv_m1_kernel(const unsigned short* __restrict__ X,
                     const unsigned char* __restrict__ W,
                     const float* __restrict__ S,
                     unsigned short* __restrict__ Y, int N, int K,
                     int group) {
  constexpr int KPL = BITS == 8 ? 16 : 32;       // weights per 16-B piece
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const long rowb = BITS == 8 ? (long)K : (long)(K >> 1);   // bytes per row
  const int G = BITS == 8 ? 1 : K / group;       // scales per row
  const long wstride = (long)gridDim.x * (4 * RPW);
  for (long n0 = (long)blockIdx.x * (4 * RPW) + wid * RPW; n0 < N;
       n0 += wstride) {
    // rows past N-1 alias onto row n0: loads stay in bounds, no store
    long rn[RPW];
    const unsigned char* wr[RPW];
    float acc[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      rn[r] = n0 + r < N ? n0 + r : n0;
      wr[r] = W + rn[r] * rowb;
      acc[r] = 0.f;
    }
#pragma unroll 2
    for (int k = lane * KPL; k < K; k += 64 * KPL) {
      uint4q wv[RPW];
#pragma unroll
      for (int r = 0; r < RPW; ++r)
        wv[r] = *reinterpret_cast<const uint4q*>(
            wr[r] + (BITS == 8 ? k : (k >> 1)));
      uint4q xq[KPL / 8];                        // x as packed bf16 pairs
#pragma unroll
      for (int i = 0; i < KPL / 8; ++i)
        xq[i] = *reinterpret_cast<const uint4q*>(X + k + 8 * i);
      if (BITS == 8) {
        float xv[KPL];
#pragma unroll
        for (int i = 0; i < KPL / 2; ++i) {
          xv[2 * i] = __uint_as_float(xq[i >> 2][i & 3] << 16);
          xv[2 * i + 1] = __uint_as_float(xq[i >> 2][i & 3] & 0xffff0000u);
        }
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
          float p = 0.f;
#pragma unroll
          for (int d = 0; d < 4; ++d) {
#pragma unroll
            for (int b = 0; b < 4; ++b)
              p += xv[4 * d + b] * qg_sbyte(wv[r][d], b);
          }
          acc[r] += p;
        }
      } else {
        // Nibbles go to bf16 with two integer ops per pair: 0x4300 | nib
        // is the bf16 128 + nib, exactly. (p >> 4j) & 0x000F000F pairs
        // nibble j with nibble j + 4, so x is permuted to the same
        // pairs once per step (shared by the RPW rows) and both feed
        // v_dot2c_f32_bf16 — x is never widened to fp32. The stored
        // nibble is q + 8, so the lane's partial sum is
        // sum x*(128 + nib) - 136 * sum x, scaled by its one group.
        float sx = 0.f;
        unsigned xp[16];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          xp[4 * d + 0] = __builtin_amdgcn_perm(xq[d][2], xq[d][0], 0x05040100u);
          xp[4 * d + 1] = __builtin_amdgcn_perm(xq[d][2], xq[d][0], 0x07060302u);
          xp[4 * d + 2] = __builtin_amdgcn_perm(xq[d][3], xq[d][1], 0x05040100u);
          xp[4 * d + 3] = __builtin_amdgcn_perm(xq[d][3], xq[d][1], 0x07060302u);
#pragma unroll
          for (int i = 0; i < 4; ++i) sx = qg_dot2(xq[d][i], 0x3F803F80u, sx);
        }
        const int g = k / group;
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
          float p = 0.f;
#pragma unroll
          for (int d = 0; d < 4; ++d) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              p = qg_dot2(((wv[r][d] >> (4 * j)) & 0x000F000Fu) | 0x43004300u,
                          xp[4 * d + j], p);
          }
          acc[r] += (p - 136.f * sx) * S[rn[r] * G + g];
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      float v = wave_reduce_sum(acc[r]);
      if (BITS == 8) v *= S[rn[r]];
      if (lane == r && n0 + r < N) Y[n0 + r] = f2bf(v);
    }
  }
}

// ----------------------------------------------------- (b) 2 <= M <= 16
// Block = NW waves sharing T 16-row tiles; wave w takes k-steps w, w+NW,
// ... of 4 pieces (one per lane quad). D layout of the 16x16x32 MFMA:
// col (batch row m) = lane & 15, row (weight row) = 4*(lane >> 4) + reg.
// GPS (int4): scale groups per 128-k wave step — 1 (group % 128 == 0),
// 2 (group 64) or 4 (any other group % 32 == 0: one group per piece).
template <int BITS, int T, int NW, int GPS>
__global__ __launch_bounds__(NW * 64)
void qgemm_mfma_kernel(const unsigned short* __restrict__ X,
                       const unsigned char* __restrict__ W,
                       const float* __restrict__ S,
                       unsigned short* __restrict__ Y, int M, int N, int K,
                       int group) {
  constexpr int KPL = BITS == 8 ? 16 : 32;       // weights per 16-B piece
  constexpr int STEP = 4 * KPL;                  // k per wave step
  __shared__ float red[NW * T * 256];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int r = lane & 15, h = lane >> 4;
  const long rowb = BITS == 8 ? (long)K : (long)(K >> 1);
  const int G = BITS == 8 ? 1 : K / group;
  const long n0 = (long)blockIdx.x * (16 * T);

  const unsigned char* wr[T];
  long rs[T][4];                                 // rows of this lane's D regs
  float4v acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const long n = n0 + t * 16 + r;
    // never address past N-1: tail rows alias the last row, not stored
    wr[t] = W + (n < N ? n : (long)N - 1) * rowb;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long ns = n0 + t * 16 + 4 * h + e;
      rs[t][e] = ns < N ? ns : (long)N - 1;
    }
    acc[t] = (float4v){0.f, 0.f, 0.f, 0.f};
  }
  const bool mrow = r < M;                       // batch rows >= M: zeros
  const unsigned short* xr = X + (long)(mrow ? r : 0) * K;

  // wave-uniform trip count: every lane reaches every MFMA
#pragma unroll 2
  for (int kb = wid * STEP; kb < K; kb += NW * STEP) {
    const int k = kb + h * KPL;
    const bool kin = k < K;                      // whole piece in or out
    uint4q wv[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      // pieces past K: q = 0 (int4 stores q + 8)
      wv[t] = BITS == 8 ? (uint4q){0u, 0u, 0u, 0u}
                        : (uint4q){0x88888888u, 0x88888888u, 0x88888888u,
                                   0x88888888u};
      if (kin)
        wv[t] = *reinterpret_cast<const uint4q*>(
            wr[t] + (BITS == 8 ? k : (k >> 1)));
    }
    short8v xf[KPL / 8];
#pragma unroll
    for (int i = 0; i < KPL / 8; ++i) {
      xf[i] = (short8v){0, 0, 0, 0, 0, 0, 0, 0};
      if (kin && mrow)
        xf[i] = *reinterpret_cast<const short8v*>(xr + k + 8 * i);
    }
    if (BITS == 8) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {            // 8 k per fragment
          union { unsigned u[4]; short8v v; } a;
#pragma unroll
          for (int d = 0; d < 2; ++d) {
            const unsigned u = wv[t][2 * j + d];
            // |q| <= 127 is exact in bf16
            a.u[2 * d] = qg_pack_bf16(qg_sbyte(u, 0), qg_sbyte(u, 1));
            a.u[2 * d + 1] = qg_pack_bf16(qg_sbyte(u, 2), qg_sbyte(u, 3));
          }
          acc[t] = MFMA16(a.v, xf[j], acc[t]);
        }
      }
    } else {
      // Exact weights, fp32 scales. As in the M = 1 kernel a nibble
      // becomes the bf16 128 + nib with integer ops, which pairs k j
      // with k j + 4 inside a dword, so the x fragments are permuted to
      // the same pairing once per step. Each scale group of the step
      // gets a fresh accumulator (the x fragments of the other groups'
      // lane quads masked to zero) plus the group's sum of x from an
      // all-ones A operand (shared by the T tiles), and
      // (sum x*(128 + nib) - 136 * sum x) is scaled per weight row in
      // fp32 — the M = 1 kernel's rounding.
      constexpr int QPG = 4 / GPS;               // lane quads per group
      short8v xm[GPS][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        union { unsigned u[4]; short8v v; } xi, xo;
        xi.v = xf[j];
        xo.u[0] = __builtin_amdgcn_perm(xi.u[2], xi.u[0], 0x05040100u);
        xo.u[1] = __builtin_amdgcn_perm(xi.u[2], xi.u[0], 0x07060302u);
        xo.u[2] = __builtin_amdgcn_perm(xi.u[3], xi.u[1], 0x05040100u);
        xo.u[3] = __builtin_amdgcn_perm(xi.u[3], xi.u[1], 0x07060302u);
#pragma unroll
        for (int u = 0; u < GPS; ++u)
          xm[u][j] = (GPS == 1 || h / QPG == u)
                         ? xo.v : (short8v){0, 0, 0, 0, 0, 0, 0, 0};
      }
      union { unsigned u[4]; short8v v; } ones;
#pragma unroll
      for (int i = 0; i < 4; ++i) ones.u[i] = 0x3F803F80u;
      float4v sxu[GPS];                          // sum x per (m, group)
#pragma unroll
      for (int u = 0; u < GPS; ++u) {
        sxu[u] = (float4v){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j)
          sxu[u] = MFMA16(ones.v, xm[u][j], sxu[u]);
      }
#pragma unroll
      for (int t = 0; t < T; ++t) {
        float4v part[GPS];
#pragma unroll
        for (int u = 0; u < GPS; ++u)
          part[u] = (float4v){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {            // one dword = 8 k
          union { unsigned u[4]; short8v v; } a;
#pragma unroll
          for (int i = 0; i < 4; ++i)
            a.u[i] = ((wv[t][j] >> (4 * i)) & 0x000F000Fu) | 0x43004300u;
#pragma unroll
          for (int u = 0; u < GPS; ++u)
            part[u] = MFMA16(a.v, xm[u][j], part[u]);
        }
#pragma unroll
        for (int u = 0; u < GPS; ++u) {
          // group of quads u*QPG..: wave-uniform; a group past K has
          // only zero partials, its scale index is clamped in range
          int g = (kb + u * QPG * KPL) / group;
          g = g < G ? g : G - 1;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            acc[t][e] += S[rs[t][e] * G + g] *
                         (part[u][e] - 136.f * sxu[u][e]);
        }
      }
    }
  }

  // cross-wave K reduction in LDS, then scale (int8) and store rows < M
#pragma unroll
  for (int t = 0; t < T; ++t)
    *reinterpret_cast<float4v*>(&red[((wid * T + t) * 64 + lane) * 4]) =
        acc[t];
  __syncthreads();
  for (int e = threadIdx.x; e < T * 256; e += NW * 64) {
    const int t = e >> 8;
    const int m = (e >> 4) & 15;
    const int nl = e & 15;                       // consecutive threads:
    const int src = ((nl >> 2) * 16 + m) * 4 + (nl & 3);   // consecutive n
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) v += red[(w * T + t) * 256 + src];
    const long n = n0 + t * 16 + nl;
    if (m < M && n < N) {
      if (BITS == 8) v *= S[n];
      Y[(long)m * N + n] = f2bf(v);
    }
  }
}

// --------------------------------------------------------------- launch
template <int BITS, int RPW>
static void qgemv_m1_launch(const void* x, const void* w, const float* s,
                            void* y, int N, int K, int group,
                            hipStream_t st) {
  long blocks = DTX_CDIV((long)N, 4 * RPW);
  int grid = (int)(blocks < 4096 ? (blocks < 1 ? 1 : blocks) : 4096);
  qgemv_m1_kernel<BITS, RPW><<<grid, DTX_BLOCK, 0, st>>>(
      (const unsigned short*)x, (const unsigned char*)w, s,
      (unsigned short*)y, N, K, group);
}

template <int BITS, int T, int GPS>
static void qgemm_mfma_launch_g(const void* x, const void* w,
                                const float* s, void* y, int M, int N,
                                int K, int group, hipStream_t st) {
  constexpr int NW = 8;
  const int grid = (int)DTX_CDIV((long)N, 16 * T);
  qgemm_mfma_kernel<BITS, T, NW, GPS><<<grid, NW * 64, 0, st>>>(
      (const unsigned short*)x, (const unsigned char*)w, s,
      (unsigned short*)y, M, N, K, group);
}

template <int BITS, int T>
static void qgemm_mfma_launch(const void* x, const void* w, const float* s,
                              void* y, int M, int N, int K, int group,
                              hipStream_t st) {
  if (BITS == 8 || group % 128 == 0)
    qgemm_mfma_launch_g<BITS, T, 1>(x, w, s, y, M, N, K, group, st);
  else if (group == 64)
    qgemm_mfma_launch_g<BITS, T, 2>(x, w, s, y, M, N, K, group, st);
  else
    qgemm_mfma_launch_g<BITS, T, 4>(x, w, s, y, M, N, K, group, st);
}

template <int BITS>
static void qgemv_dispatch(const void* x, const void* w, const float* s,
                           void* y, int M, int N, int K, int group,
                           hipStream_t st) {
  if (M == 1) {
    // rows per wave from N: 256 CUs want >= ~512 four-wave blocks
    if (N >= 16384)
      qgemv_m1_launch<BITS, 4>(x, w, s, y, N, K, group, st);
    else if (N >= 4096)
      qgemv_m1_launch<BITS, 2>(x, w, s, y, N, K, group, st);
    else
      qgemv_m1_launch<BITS, 1>(x, w, s, y, N, K, group, st);
    return;
  }
  // tiles per x fragment from N: keep >= ~256 blocks, then amortize the
  // x re-read (M*2 bytes per k against 16*T weights)
  if (N >= 16384)
    qgemm_mfma_launch<BITS, 4>(x, w, s, y, M, N, K, group, st);
  else if (N >= 8192)
    qgemm_mfma_launch<BITS, 2>(x, w, s, y, M, N, K, group, st);
  else
    qgemm_mfma_launch<BITS, 1>(x, w, s, y, M, N, K, group, st);
}

void launch_qgemv_int8(const void* x, const void* q, const float* scale,
                       void* y, int M, int N, int K, hipStream_t st) {
  qgemv_dispatch<8>(x, q, scale, y, M, N, K, K, st);
}

void launch_qgemv_int4(const void* x, const void* packed,
                       const float* scale, void* y, int M, int N, int K,
                       int group, hipStream_t st) {
  qgemv_dispatch<4>(x, packed, scale, y, M, N, K, group, st);
}
