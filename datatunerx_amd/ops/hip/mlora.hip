// Batched gathered LoRA update for decode rows (multi-adapter serving):
// every row of the batch picks its own adapter out of a stack.
//
//   y[m,:] = bf16(float(y[m,:]) + scale[g] * ((x[m,:] . A[g]^T) . Bt[g])),
//   g = idx[m]
//
// x [M,K], y [M,N] bf16; A [G,R,K], Bt [G,R,N] bf16 (B stored
// pre-transposed, ranks zero-padded to the stack's common R); scale [G]
// f32; idx [M] int32 ON THE DEVICE. A row whose index is outside [0,G)
// is skipped by both kernels before anything of A/Bt is addressed: y
// keeps its bits and t[m,:] is never read (it stays uninitialised).
//
// idx is only ever read by the kernels, so one captured graph serves
// every later assignment of adapters. No atomics, no workspace to clear.
//
// A row's result depends on that row alone: the grid's y dimension is
// the row, nothing is tiled across rows, and the summation order of a
// row is fixed by (K, N) only — a mixed batch equals, bit for bit, the
// same rows run one at a time. The order is also independent of R: t[j]
// is summed the same way whatever the stack's rank, and the expand sums
// j = 0..R-1 in one chain, so zero-padded ranks only add exact zeros.
//
//   shrink:  t[m,j] = x[m,:] . A[g,j,:]  (fp32). A block owns RJ ranks
//            of one row; its 4 waves interleave over K in 16-byte
//            pieces (the block reads 4 KB contiguous per rank per step),
//            wave-shuffle reduction, then 4 partials per rank meet in
//            LDS and are added in a fixed order.
//   expand:  one wave per 512 columns of one row; each lane owns 8
//            columns (one 16-byte load per rank, coalesced along N), t
//            is lane-uniform, fp32 accumulate, one bf16 rounding of
//            y + scale * acc.
// Both are a few microseconds of latency-bound work per projection: the
// grids are shaped to spread one row's adapter (R*K*2 bytes) over many
// waves rather than to reuse anything between rows.
#include "dtx_common.h"
#include "dtx_launch.h"

template <int RJ>
__global__ __launch_bounds__(DTX_BLOCK)
void mlora_shrink_kernel(const unsigned short* __restrict__ X,
                         const unsigned short* __restrict__ A,
                         const int* __restrict__ idx,
                         float* __restrict__ T, int K, int R, int G) {
  __shared__ float red[4][RJ];
  const int m = blockIdx.y;
  const int g = idx[m];
  if (g < 0 || g >= G) return;                   // block-uniform
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int j0 = blockIdx.x * RJ;                // R % RJ == 0 (launcher)
  const unsigned short* xr = X + (long)m * K;
  const unsigned short* ar = A + ((long)g * R + j0) * K;
  float acc[RJ];
#pragma unroll
  for (int j = 0; j < RJ; ++j) acc[j] = 0.f;
  // K % 8 == 0: a lane's 8-element piece is wholly inside K or skipped
#pragma unroll 2
  for (int k = threadIdx.x * 8; k < K; k += DTX_BLOCK * 8) {
    float xv[8];
    load_bf16x8(xr + k, xv);
#pragma unroll
    for (int j = 0; j < RJ; ++j) {
      float av[8];
      load_bf16x8(ar + (long)j * K + k, av);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[j] += xv[i] * av[i];
    }
  }
#pragma unroll
  for (int j = 0; j < RJ; ++j) {
    const float v = wave_reduce_sum(acc[j]);
    if (lane == 0) red[wid][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < RJ) {
    const int j = threadIdx.x;
    T[(long)m * R + j0 + j] =
        (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
  }
}

template <int R>
__global__ __launch_bounds__(WAVE)
void mlora_expand_add_kernel(unsigned short* __restrict__ Y,
                             const float* __restrict__ T,
                             const unsigned short* __restrict__ Bt,
                             const float* __restrict__ S,
                             const int* __restrict__ idx, int N, int G) {
  const int m = blockIdx.y;
  const int g = idx[m];
  if (g < 0 || g >= G) return;                   // block-uniform
  const long n = ((long)blockIdx.x * WAVE + threadIdx.x) * 8;
  if (n >= N) return;                            // N % 8 == 0
  const float* tr = T + (long)m * R;
  const unsigned short* br = Bt + (long)g * R * N + n;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 8
  for (int j = 0; j < R; ++j) {
    const float t = tr[j];                       // lane-uniform
    float w[8];
    load_bf16x8(br + (long)j * N, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += t * w[i];
  }
  const float s = S[g];
  unsigned short* yp = Y + (long)m * N + n;
  float y[8];
  load_bf16x8(yp, y);
#pragma unroll
  for (int i = 0; i < 8; ++i) y[i] += s * acc[i];
  store_bf16x8(yp, y);
}

// ------------------------------------------------------------- launchers
// R in {8, 16, 32, 64}; 1 <= M <= 16; K % 8 == 0; N % 8 == 0 (checked by
// the binding). idx is a device pointer and is never read here.
void launch_mlora_shrink(const void* x, const void* a, const int* idx,
                         float* t, int M, int K, int R, int G,
                         hipStream_t s) {
  // ranks per block: 2 for the small ranks (R = 8 still gives 4 blocks
  // a row), 4 above (x is re-read by R / RJ blocks, from L2)
  if (R <= 16) {
    dim3 grid(R / 2, M);
    mlora_shrink_kernel<2><<<grid, DTX_BLOCK, 0, s>>>(
        (const unsigned short*)x, (const unsigned short*)a, idx, t, K, R,
        G);
  } else {
    dim3 grid(R / 4, M);
    mlora_shrink_kernel<4><<<grid, DTX_BLOCK, 0, s>>>(
        (const unsigned short*)x, (const unsigned short*)a, idx, t, K, R,
        G);
  }
}

void launch_mlora_expand_add(void* y, const float* t, const void* bt,
                             const float* scale, const int* idx, int M,
                             int N, int R, int G, hipStream_t s) {
  dim3 grid(DTX_CDIV(N, WAVE * 8), M);
#define MLORA_EX(RC)                                                      \
  mlora_expand_add_kernel<RC><<<grid, WAVE, 0, s>>>(                      \
      (unsigned short*)y, t, (const unsigned short*)bt, scale, idx, N, G)
  if (R == 8) MLORA_EX(8);
  else if (R == 16) MLORA_EX(16);
  else if (R == 32) MLORA_EX(32);
  else MLORA_EX(64);
#undef MLORA_EX
}
