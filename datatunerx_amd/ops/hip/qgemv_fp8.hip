// Weight-streaming e4m3 GEMM for 1..16 rows (gfx950): the decode step of a
// model whose frozen base is stored in fp8 (models/quant.py, codebook
// "e4m3"), in the arithmetic the fp8 base GEMMs train and prefill in.
//   y[M,N] = bf16(sa[m] * sw[n] * sum_k x8[m,k] * w8[n,k])    1 <= M <= 16
//   (x8, sa) = quant_fp8_rows(x), formed inside the kernel from bf16 x
//   w8 [N,K] e4m3 row-major, sw [N] f32 (quant_fp8_rows of the weight)
// K % 128 == 0, 128 <= K <= quant_fp8_max_k(), any N >= 1; fp32 accumulate,
// both scales applied in fp32 in the epilogue, one rounding to bf16.
//
// Operands. The 16 weight rows of a tile are the A operand of
// v_mfma_scale_f32_16x16x128_f8f6f4 (unit hardware scales, gemm_fp8.hip's
// MFMA_F8), the batch rows the B operand, zero-padded to 16 in registers.
// The contraction is permuted as in skinny.hip: in a k-step of 128, lane
// (row r = lane & 15, quad h = lane >> 4) takes the contiguous 32 bytes
// h of weight row r and the same 32 k of x row r, so both operands agree
// and every weight load is contiguous. One MFMA consumes 2 KB of weight.
//
// K walk: skinny.hip's plan in bytes. K is cut into batches of FQ_STEPS = 4
// k-steps (512 k, 512 contiguous bytes of a weight row, the bytes of
// skinny's batch). A block's 8 waves take batches w, w + 8, ... A wave's
// unit of work is (batch, tile): the loads of the NEXT unit are issued
// before the 4 MFMAs of the current one, so a wave always holds one unit
// (8 KB) in flight; the first unit goes out before the quantizer's first
// pass. T row tiles share one x operand. Weight loads are unconditional:
// rows clamp to N-1, k clamps to K-32. A k-step is wholly inside K or
// wholly past it (K % 128 == 0), wave-uniformly, and a step past K issues
// no MFMA. Batch rows >= M become zero by a select at the MFMA, never at
// a load (docs/kernels.md, "The waitcnt trap").
//
// Activation quantization, in the kernel, bit for bit quant_fp8_rows:
//  1. absmax. The 512 threads split each live row's K in 16-byte pieces,
//     reduce in the wave, and the 8 waves meet in LDS (max is exact in any
//     order). s = amax > 0 ? amax / 448 : 1 once per row, kept in LDS for
//     the convert and the epilogue.
//  2. convert, per wave for its own batches, staged through a wave-private
//     LDS slab of [16 rows][512 B]. Chosen over a block-wide x8 copy
//     because M * K bytes do not fit at the shapes that matter (16 rows of
//     an 11008-wide down projection are 172 KB), and over converting in
//     the MFMA layout because there every lane converts its row's 32 k of
//     every step whether or not the row is live: the IEEE division chain is
//     ~10 VALU ops per element, 16 rows' worth per step even at M = 1. In
//     the slab pass m (m < M, wave-uniform) lane l converts the 8 k of
//     piece l of row m — x / s, clamp to +-448, cvt_pk_fp8_f32, the
//     quantizer's operations in its order — so the cost scales with M. The
//     B fragments of the batch are then two 16-byte LDS reads per step
//     (row stride padded by 16 B against bank conflicts) and serve all T
//     tiles. Rows >= M of the slab are never written; their lanes are the
//     ones the select zeroes.
//
// Reduction. The 8 partial accumulators of an output meet in LDS (the
// slabs' memory, reused behind a barrier) and are summed in wave order
// 0..7: no workspace, no memset, no atomic. An output's sum is: per wave,
// batches w, w+8, ... in order, each k-step one MFMA; then the waves in
// order. That order and the grid depend on (N, K) only; a column of D reads
// its own column of B and a row's scale its own row of x: a row's bits do
// not depend on M or on the other rows of its batch.
//
// Tails: rows past N-1 alias row N-1 for loads and are never stored. Row
// offsets are long.
//
// Build: no packed fp32 VALU instructions, as in skinny.hip; thread and
// block ids come from the builtins.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                              \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "dtx_mfma.h"
#include "dtx_launch.h"

typedef __attribute__((ext_vector_type(8))) int int8v;
typedef __attribute__((ext_vector_type(4))) int int4v;
typedef __attribute__((ext_vector_type(2))) unsigned uint2v;

#define FP8_MAX 448.f
#define MFMA_F8(a, b, c)                                                   \
  __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0,       \
                                                   0x7f7f7f7f, 0, 0x7f7f7f7f)

#define FQ_TID ((int)__builtin_amdgcn_workitem_id_x())
#define FQ_BID ((int)__builtin_amdgcn_workgroup_id_x())
#define FQ_NW 8                      // waves per block
#define FQ_STEPS 4                   // k-steps per batch
#define FQ_BATCH (128 * FQ_STEPS)    // k (= weight bytes of a row) per batch
#define FQ_ROWB (FQ_BATCH + 16)      // slab row stride in bytes
#define FQ_SLAB (16 * FQ_ROWB)       // one wave's slab

// the FQ_STEPS 32-byte pieces of one (batch, tile) unit; kb = first k of
// the batch. `base` is block-uniform and `row` this lane's 32-bit byte
// offset from it (at most 64 rows of K <= 2^14).
__device__ __forceinline__ void fq_load(int8v (&f)[FQ_STEPS],
                                        const unsigned char* base,
                                        unsigned row, int kb, int h, int K) {
#pragma unroll
  for (int s = 0; s < FQ_STEPS; ++s) {
    const int k = kb + s * 128 + h * 32;
    const int4v* p = reinterpret_cast<const int4v*>(
        base + (row + (unsigned)(k < K ? k : K - 32)));
    const int4v lo = p[0], hi = p[1];
    f[s] = int8v{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  }
}

template <int T>
__global__ __launch_bounds__(FQ_NW * 64)
void qgemv_fp8_kernel(const unsigned short* __restrict__ X,
                      const unsigned char* __restrict__ W,
                      const float* __restrict__ SW,
                      unsigned short* __restrict__ Y, int M, int N, int K) {
  static_assert(FQ_NW * T * 256 * 4 <= FQ_NW * FQ_SLAB, "red fits the slabs");
  __shared__ __attribute__((aligned(16))) unsigned char slab[FQ_NW * FQ_SLAB];
  __shared__ float amx[FQ_NW * 16];            // per wave, per row absmax
  __shared__ float sa[16];                     // row scales
  const int tid = FQ_TID;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, h = lane >> 4;
  const long n0 = (long)FQ_BID * (16 * T);

  // n0 <= N-1 for every block of the grid
  const unsigned char* wb = W + n0 * K;        // block-uniform, long offset
  unsigned wr[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const long n = n0 + t * 16 + r;
    // never address past N-1: tail rows alias the last row, not stored
    wr[t] = (unsigned)((n < N ? n : (long)N - 1) - n0) * (unsigned)K;
  }
  const bool mrow = r < M;                     // batch rows >= M: zeros

  // the first unit's weights are in flight through the absmax pass
  int8v wbuf[2][FQ_STEPS];
  fq_load(wbuf[0], wb, wr[0], wid * FQ_BATCH, h, K);

  // ---- 1. row absmax over all of K: threads split K, waves meet in LDS
  for (int m = 0; m < M; ++m) {
    const unsigned short* xr = X + (unsigned)m * (unsigned)K;
    float a = 0.f;
    for (int k = tid * 8; k < K; k += FQ_NW * 64 * 8) {
      const short8v v = *reinterpret_cast<const short8v*>(xr + k);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        a = fmaxf(a, fabsf(bf2f((unsigned short)v[j])));
    }
    a = wave_reduce_max(a);
    if (lane == 0) amx[wid * 16 + m] = a;
  }
  __syncthreads();
  if (tid < M) {
    float a = 0.f;
#pragma unroll
    for (int w = 0; w < FQ_NW; ++w) a = fmaxf(a, amx[w * 16 + tid]);
    sa[tid] = a > 0.f ? a / FP8_MAX : 1.f;
  }
  __syncthreads();

  float4v acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = (float4v){0.f, 0.f, 0.f, 0.f};

  // Units alternate between two register buffers, so a loop iteration
  // holds an even number of units: one batch when T is even, two batches
  // when T == 1 — there the second may lie past K, where no step issues
  // an MFMA.
  constexpr int BPI = T == 1 ? 2 : 1;          // batches per iteration
  const int NB = DTX_CDIV(K, FQ_BATCH);
  const int8v z8 = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned char* my = slab + wid * FQ_SLAB;    // this wave's slab
  for (int b = wid; b < NB; b += BPI * FQ_NW) {   // wave-uniform trip count
#pragma unroll
    for (int i = 0; i < BPI; ++i) {
      const int kb = (b + i * FQ_NW) * FQ_BATCH;
      // ---- 2. quantize the batch's x into the slab: pass m is row m,
      // lane l its piece l (k clamps to K-8; a piece past K belongs to a
      // step that issues no MFMA)
      const int kx = kb + lane * 8;
      const unsigned xo = (unsigned)(kx < K ? kx : K - 8);
      for (int m = 0; m < M; ++m) {
        const short8v v = *reinterpret_cast<const short8v*>(
            X + ((unsigned)m * (unsigned)K + xo));
        const float s = sa[m];
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          f[j] = fminf(fmaxf(bf2f((unsigned short)v[j]) / s, -FP8_MAX),
                       FP8_MAX);
        int lo = 0, hi = 0;
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
        uint2v o; o.x = (unsigned)lo; o.y = (unsigned)hi;
        *reinterpret_cast<uint2v*>(my + m * FQ_ROWB + lane * 8) = o;
      }
      // the slab is the wave's own: its writes before its reads
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      int8v xq[FQ_STEPS];
#pragma unroll
      for (int s = 0; s < FQ_STEPS; ++s) {
        const int4v* p = reinterpret_cast<const int4v*>(
            my + r * FQ_ROWB + s * 128 + h * 32);
        const int4v lo = p[0], hi = p[1];
        xq[s] = mrow ? int8v{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}
                     : z8;
      }
      // the next batch's passes write the slab only behind these reads
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const int u = (i * T + t) & 1;         // this unit's buffer
        // the next unit's loads go out before this unit's MFMAs
        if (t + 1 < T)
          fq_load(wbuf[u ^ 1], wb, wr[t + 1], kb, h, K);
        else
          fq_load(wbuf[u ^ 1], wb, wr[0], kb + FQ_NW * FQ_BATCH, h, K);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < FQ_STEPS; ++s)
          if (kb + s * 128 < K)                // wave-uniform
            acc[t] = MFMA_F8(wbuf[u][s], xq[s], acc[t]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  // D layout: col (batch row m) = lane & 15, row (weight row) = 4 * h + reg
  __syncthreads();                             // every wave is done with its slab
  float* red = reinterpret_cast<float*>(slab);
#pragma unroll
  for (int t = 0; t < T; ++t)
    *reinterpret_cast<float4v*>(&red[((wid * T + t) * 64 + lane) * 4]) =
        acc[t];
  __syncthreads();
  for (int e = tid; e < T * 256; e += FQ_NW * 64) {
    const int t = e >> 8;
    const int m = (e >> 4) & 15;
    const int nl = e & 15;                       // consecutive threads:
    const int src = ((nl >> 2) * 16 + m) * 4 + (nl & 3);   // consecutive n
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < FQ_NW; ++w)              // fixed wave order
      v += red[(w * T + t) * 256 + src];
    const long n = n0 + t * 16 + nl;
    if (m < M && n < N) Y[(long)m * N + n] = f2bf(v * sa[m] * SW[n]);
  }
}

// ------------------------------------------------------------------ launch
// The one contract, shared by the binding and Python.
bool qgemv_fp8_supported(long M, long N, long K) {
  return M >= 1 && M <= 16 && N >= 1 && N <= (1L << 30) && K >= 128 &&
         K % 128 == 0 && K <= quant_fp8_max_k();
}

// Tiles per x operand from N alone, skinny.hip's rule: the x re-read and
// re-quantization is what a block pays per batch, so T = 4 as soon as N
// leaves enough blocks for the chip.
void launch_qgemv_fp8(const void* x, const void* w8, const float* sw,
                      void* y, int M, int N, int K, hipStream_t st) {
#define FQ_GO(T_)                                                          \
  qgemv_fp8_kernel<T_><<<(unsigned)DTX_CDIV((long)N, 16 * T_), FQ_NW * 64, \
                         0, st>>>((const unsigned short*)x,                \
                                  (const unsigned char*)w8, sw,            \
                                  (unsigned short*)y, M, N, K)
  if (N >= 8192) FQ_GO(4); else FQ_GO(1);
#undef FQ_GO
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
