// Weight-streaming decode kernels for NF4 base weights (gfx950):
//   y[M,N] = x[M,K] @ (level[idx] * absmax)[N,K]^T, x/y bf16, fp32
// accumulate, M <= 16. Format (models/quant.py): packed [N,K/2] uint8,
// low nibble = even k, nibble = index into the 16 NF4 levels; absmax
// [N,K/group] f32. The packed weight is streamed once with 16-byte loads;
// no bf16 weight is written to HBM.
//
// A codebook has no integer trick (qgemv.hip turns an int4 nibble into a
// bf16 with one OR), so the decode step is a table lookup by the whole
// weight BYTE: a 256-entry table of packed bf16 pairs in LDS,
//   T[b] = bf16(level[b & 15]) | bf16(level[b >> 4]) << 16,
// one ds_read_b32 per byte. The pair is already in natural k order (even
// k in the low half), so it meets the x dword exactly as loaded: no x
// permutation, no +8 bias and no sum of x. Per weight that is ~1 VALU op
// of address formation, half a dot2 / a 64th of an MFMA, half an LDS
// read. The 1 KB table is built once per block from the 16 constants.
// It is not replicated: interleaved copies (entry * R + lane % R, R = 4
// and 16) that spread a wave's random byte values over more LDS banks
// measured the same as R = 1 within the window spread at every shape
// (profiles/README.md, "NF4 decode").
//
// (a) M == 1: the shape of qgemv_m1_kernel — a wave owns RPW rows, a lane
//     takes one 16-byte piece (32 weights) per row per step, feeds
//     v_dot2c_f32_bf16, and scales its 32-weight partial by its one
//     group's absmax in fp32 (group % 32 == 0); wave reduction at the end.
// (b) 2 <= M <= 16: the structure of qgemm_mfma_kernel — 16 weight rows
//     are the A operand of mfma_f32_16x16x32_bf16, the zero-padded batch
//     rows the B operand, lane (r, h) takes the contiguous 16-byte piece
//     h, NW waves split K, T tiles share each x fragment. One packed
//     dword is four lookups = 8 bf16 of an A fragment in natural k order.
//     Every scale group of a step gets a fresh accumulator (GPS 1/2/4 from
//     `group`), scaled per weight row in fp32 and added — the M = 1
//     kernel's rounding, so M = 1 and M > 1 differ only in fp32 summation
//     order. The table and the cross-wave reduction buffer share the
//     block's LDS (no workspace, no memset: hipGraph-capturable).
//
// Tails: rows past N-1 alias onto a valid row for loads and are never
// stored; pieces past K load nothing and meet zero x; batch rows >= M are
// zeros in registers. Row offsets are long.
#include "dtx_mfma.h"
#include "dtx_launch.h"
#include "dtx_nf4.h"

typedef __attribute__((ext_vector_type(4))) unsigned nf_u32x4;
typedef __attribute__((ext_vector_type(2))) __bf16 nf_bf16x2;

// c + a.lo*b.lo + a.hi*b.hi on packed bf16 pairs (v_dot2c_f32_bf16)
__device__ __forceinline__ float nf_dot2(unsigned a, unsigned b, float c) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(nf_bf16x2, a),
                                         __builtin_bit_cast(nf_bf16x2, b),
                                         c, false);
}

// Fill tab[256] (all threads of the block; ends in a barrier)
__device__ __forceinline__ void nf4_build_table(unsigned* tab) {
  for (int b = threadIdx.x; b < 256; b += blockDim.x)
    tab[b] = (unsigned)f2bf(dtx_nf4_level(b & 15)) |
             (unsigned)f2bf(dtx_nf4_level(b >> 4)) << 16;
  __syncthreads();
}

// packed bf16 pair of byte j of dword p
__device__ __forceinline__ unsigned nf4_pair(const unsigned* tab, unsigned p,
                                             int j) {
  return tab[(p >> (8 * j)) & 0xffu];
}

// ------------------------------------------------------------ (a) M = 1
template <int RPW>
__global__ __launch_bounds__(DTX_BLOCK)
void qgemv_nf4_m1_kernel(const unsigned short* __restrict__ X,
                         const unsigned char* __restrict__ W,
                         const float* __restrict__ S,
                         unsigned short* __restrict__ Y, int N, int K,
                         int group) {
  __shared__ unsigned tab[256];
  nf4_build_table(tab);
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const long rowb = (long)(K >> 1);              // bytes per row
  const int G = K / group;                       // scales per row
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
    for (int k = lane * 32; k < K; k += 64 * 32) {
      nf_u32x4 wv[RPW];
#pragma unroll
      for (int r = 0; r < RPW; ++r)
        wv[r] = *reinterpret_cast<const nf_u32x4*>(wr[r] + (k >> 1));
      nf_u32x4 xq[4];                            // x as packed bf16 pairs
#pragma unroll
      for (int i = 0; i < 4; ++i)
        xq[i] = *reinterpret_cast<const nf_u32x4*>(X + k + 8 * i);
      const int g = k / group;
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        float p = 0.f;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
#pragma unroll
          for (int j = 0; j < 4; ++j)            // byte 4d+j: k + 8d + 2j, +1
            p = nf_dot2(nf4_pair(tab, wv[r][d], j), xq[d][j], p);
        }
        acc[r] += p * S[rn[r] * G + g];
      }
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const float v = wave_reduce_sum(acc[r]);
      if (lane == r && n0 + r < N) Y[n0 + r] = f2bf(v);
    }
  }
}

// ----------------------------------------------------- (b) 2 <= M <= 16
// Block = NW waves sharing T 16-row tiles; wave w takes k-steps w, w+NW,
// ... of 4 pieces (one per lane quad). D layout of the 16x16x32 MFMA:
// col (batch row m) = lane & 15, row (weight row) = 4*(lane >> 4) + reg.
// GPS: scale groups per 128-k wave step — 1 (group % 128 == 0), 2 (group
// 64) or 4 (any other group % 32 == 0: one group per piece).
template <int T, int NW, int GPS>
__global__ __launch_bounds__(NW * 64)
void qgemm_nf4_mfma_kernel(const unsigned short* __restrict__ X,
                           const unsigned char* __restrict__ W,
                           const float* __restrict__ S,
                           unsigned short* __restrict__ Y, int M, int N,
                           int K, int group) {
  // the table (256 dwords) lives until the k loop ends, the reduction
  // buffer after it
  __shared__ float red[NW * T * 256];
  unsigned* tab = reinterpret_cast<unsigned*>(red);
  nf4_build_table(tab);
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int r = lane & 15, h = lane >> 4;
  const long rowb = (long)(K >> 1);
  const int G = K / group;
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
  for (int kb = wid * 128; kb < K; kb += NW * 128) {
    const int k = kb + h * 32;
    const bool kin = k < K;                      // whole piece in or out
    nf_u32x4 wv[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      // pieces past K: any finite level, their x fragments are zero
      wv[t] = (nf_u32x4){0u, 0u, 0u, 0u};
      if (kin)
        wv[t] = *reinterpret_cast<const nf_u32x4*>(wr[t] + (k >> 1));
    }
    // x fragments as loaded; each scale group of the step sees the
    // fragments of the other groups' lane quads as zeros
    constexpr int QPG = 4 / GPS;                 // lane quads per group
    short8v xm[GPS][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      short8v xf = (short8v){0, 0, 0, 0, 0, 0, 0, 0};
      if (kin && mrow)
        xf = *reinterpret_cast<const short8v*>(xr + k + 8 * j);
#pragma unroll
      for (int u = 0; u < GPS; ++u)
        xm[u][j] = (GPS == 1 || h / QPG == u)
                       ? xf : (short8v){0, 0, 0, 0, 0, 0, 0, 0};
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      float4v part[GPS];
#pragma unroll
      for (int u = 0; u < GPS; ++u)
        part[u] = (float4v){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j) {              // one dword = 8 k
        union { unsigned u[4]; short8v v; } a;
#pragma unroll
        for (int i = 0; i < 4; ++i) a.u[i] = nf4_pair(tab, wv[t][j], i);
#pragma unroll
        for (int u = 0; u < GPS; ++u)
          part[u] = MFMA16(a.v, xm[u][j], part[u]);
      }
#pragma unroll
      for (int u = 0; u < GPS; ++u) {
        // group of quads u*QPG..: wave-uniform; a group past K has only
        // zero partials, its scale index is clamped in range
        int g = (kb + u * QPG * 32) / group;
        g = g < G ? g : G - 1;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          acc[t][e] += S[rs[t][e] * G + g] * part[u][e];
      }
    }
  }

  // every wave is done with the table before red overwrites it; then the
  // cross-wave K reduction in LDS and the store of rows < M
  __syncthreads();
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
    if (m < M && n < N) Y[(long)m * N + n] = f2bf(v);
  }
}

// --------------------------------------------------------------- launch
template <int RPW>
static void qgemv_nf4_m1_launch(const void* x, const void* w, const float* s,
                                void* y, int N, int K, int group,
                                hipStream_t st) {
  long blocks = DTX_CDIV((long)N, 4 * RPW);
  int grid = (int)(blocks < 4096 ? (blocks < 1 ? 1 : blocks) : 4096);
  qgemv_nf4_m1_kernel<RPW><<<grid, DTX_BLOCK, 0, st>>>(
      (const unsigned short*)x, (const unsigned char*)w, s,
      (unsigned short*)y, N, K, group);
}

template <int T, int GPS>
static void qgemm_nf4_launch_g(const void* x, const void* w, const float* s,
                               void* y, int M, int N, int K, int group,
                               hipStream_t st) {
  constexpr int NW = 8;
  const int grid = (int)DTX_CDIV((long)N, 16 * T);
  qgemm_nf4_mfma_kernel<T, NW, GPS><<<grid, NW * 64, 0, st>>>(
      (const unsigned short*)x, (const unsigned char*)w, s,
      (unsigned short*)y, M, N, K, group);
}

template <int T>
static void qgemm_nf4_launch(const void* x, const void* w, const float* s,
                             void* y, int M, int N, int K, int group,
                             hipStream_t st) {
  if (group % 128 == 0)
    qgemm_nf4_launch_g<T, 1>(x, w, s, y, M, N, K, group, st);
  else if (group == 64)
    qgemm_nf4_launch_g<T, 2>(x, w, s, y, M, N, K, group, st);
  else
    qgemm_nf4_launch_g<T, 4>(x, w, s, y, M, N, K, group, st);
}

void launch_qgemv_nf4(const void* x, const void* packed, const float* absmax,
                      void* y, int M, int N, int K, int group,
                      hipStream_t st) {
  if (M == 1) {
    // rows per wave from N, as qgemv.hip: >= ~512 four-wave blocks
    if (N >= 16384)
      qgemv_nf4_m1_launch<4>(x, packed, absmax, y, N, K, group, st);
    else if (N >= 4096)
      qgemv_nf4_m1_launch<2>(x, packed, absmax, y, N, K, group, st);
    else
      qgemv_nf4_m1_launch<1>(x, packed, absmax, y, N, K, group, st);
    return;
  }
  // tiles per x fragment from N, as qgemv.hip
  if (N >= 16384)
    qgemm_nf4_launch<4>(x, packed, absmax, y, M, N, K, group, st);
  else if (N >= 8192)
    qgemm_nf4_launch<2>(x, packed, absmax, y, M, N, K, group, st);
  else
    qgemm_nf4_launch<1>(x, packed, absmax, y, M, N, K, group, st);
}
