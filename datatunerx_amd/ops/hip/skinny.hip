// Weight-streaming bf16 GEMM for 1..16 rows (gfx950): the batched decode
// step's base projections.
//   y[M,N] = bf16(x[M,K] . W[N,K]^T (+ residual[M,N]))     1 <= M <= 16
//   y[M,N] = swiglu(bf16(x . Wg^T), bf16(x . Wu^T))        (gate/up pair)
// x, W, y bf16, fp32 accumulate, K % 8 == 0, any N >= 1. W is the
// checkpoint's row-major [N,K] weight, read once in 16-byte pieces.
//
// Operands. The 16 weight rows of a tile are the A operand of
// mfma_f32_16x16x32_bf16, the batch rows the B operand, zero-padded to 16
// in registers. The contraction is permuted as in qgemv.hip: in a k-step
// of 32, lane (row r = lane & 15, quad h = lane >> 4) takes the contiguous
// 16-byte piece h of weight row r and the same piece of x row r, so both
// operands agree and every global load is one contiguous 16 B.
//
// K walk. K is cut into batches of SK_STEPS = 8 k-steps (256 k, 512
// contiguous bytes of a weight row). A block's 8 waves take batches
// w, w + 8, ... A wave's unit of work is (batch, tile): the 8 weight loads
// of the NEXT unit are issued before the 8 MFMAs of the current one, so a
// wave always holds one unit (8 KB) in flight while it computes; the x
// pieces of a batch (L1/L2 hits: x is at most 16 rows, shared by every
// block) are issued ahead of that prefetch and serve all tiles of the
// batch. Loads are unconditional: rows clamp to N-1 / M-1, k clamps to
// K-8, and a piece past K or a batch row >= M becomes zero by a select in
// BOTH operands at the MFMA, never at the load (docs/kernels.md, "The
// waitcnt trap"). Trip counts are wave-uniform (wid by readfirstlane);
// the prefetch of a unit past the end reads the clamped piece again.
//
// Block. TT tiles share each x fragment: T in {1, 2, 4} row tiles chosen
// from N alone (1 or 4 plain, 1 or 2 for the pair), twice that for the SwiGLU pair (tile t of Wg and tile t of
// Wu for the same 16 rows). The 8 partial accumulators of an output meet
// in LDS and are summed in wave order 0..7: no workspace, no memset, no
// atomic. An output element's sum is: per wave, batches w, w+8, ... in
// order, each k-step one MFMA; then the waves in order. That order and the
// grid depend on (N, K) only, not on M, not on T, not on the other batch
// rows (a column of D reads its own column of B): a row's bits do not
// depend on its batch, and a weight gives the same bits alone or in a
// grouped launch.
//
// Grouped launch. Up to SK_MAXW weights with one K (q/k/v) share a grid;
// the block index selects weight, output and N, block-uniformly.
//
// Epilogues (EPI): 0 plain; 1 + residual, one rounding of acc + residual;
// 2 SwiGLU: g and u are rounded to bf16 as the two-GEMM path would store
// them, then dtx_swiglu (the swiglu_fwd formula) — g and u never reach HBM.
//
// Tails: rows past N-1 alias row N-1 for loads and are never stored. Row
// offsets are long.
//
// Build: no packed fp32 VALU instructions, as in kvq.hip and for the
// reason given there; thread and block ids come from the builtins.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                              \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "dtx_mfma.h"
#include "dtx_launch.h"

#define SK_TID ((int)__builtin_amdgcn_workitem_id_x())
#define SK_BID ((int)__builtin_amdgcn_workgroup_id_x())
#define SK_NW 8                    // waves per block
#define SK_STEPS 8                 // k-steps per batch
#define SK_BATCH (32 * SK_STEPS)   // k per batch
#define SK_MAXW 3                  // weights per grouped launch

struct SkinnyGroup {
  const unsigned short* w;         // [N,K]
  const unsigned short* aux;       // EPI 1: residual [M,N]; EPI 2: Wu [N,K]
  unsigned short* y;               // [M,N]
  int N;
  int blk0;                        // first block of this weight
};
struct SkinnyArgs { SkinnyGroup g[SK_MAXW]; };

// the SK_STEPS pieces of one (batch, tile) unit; kb = first k of the batch
// `base` is block-uniform and `row` this lane's 32-bit element offset from
// it (at most 16 rows of K <= 2^24), so a load is a scalar base plus one
// VGPR of offset; the long part of the address lives in `base`.
__device__ __forceinline__ void sk_load(short8v (&f)[SK_STEPS],
                                        const unsigned short* base,
                                        unsigned row, int kb, int h, int K) {
#pragma unroll
  for (int s = 0; s < SK_STEPS; ++s) {
    const int k = kb + s * 32 + h * 8;
    f[s] = *reinterpret_cast<const short8v*>(
        base + (row + (unsigned)(k < K ? k : K - 8)));
  }
}

template <int T, int EPI>
__global__ __launch_bounds__(SK_NW * 64)
void skinny_gemm_kernel(const unsigned short* __restrict__ X,
                        const SkinnyArgs args, int M, int K) {
  constexpr int TT = EPI == 2 ? 2 * T : T;
  __shared__ __attribute__((aligned(16))) float red[SK_NW * TT * 256];
  const int tid = SK_TID;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, h = lane >> 4;
  const int bid = SK_BID;

  // block-uniform: which weight of the group
  const int gi = bid >= args.g[2].blk0 ? 2 : (bid >= args.g[1].blk0 ? 1 : 0);
  const SkinnyGroup G = gi == 2 ? args.g[2] : (gi == 1 ? args.g[1]
                                                       : args.g[0]);
  const int N = G.N;
  const long n0 = (long)(bid - G.blk0) * (16 * T);

  // n0 <= N-1 for every block of the grid
  const unsigned short* wb = G.w + n0 * K;   // block-uniform, long offset
  const unsigned short* ub = EPI == 2 ? G.aux + n0 * K : wb;
  unsigned wr[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    const long n = n0 + (t % T) * 16 + r;
    // never address past N-1: tail rows alias the last row, not stored
    wr[t] = (unsigned)((n < N ? n : (long)N - 1) - n0) * (unsigned)K;
  }
  const bool mrow = r < M;                   // batch rows >= M: zeros
  const unsigned xr = (unsigned)(mrow ? r : M - 1) * (unsigned)K;

  float4v acc[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) acc[t] = (float4v){0.f, 0.f, 0.f, 0.f};

  // Units alternate between two register buffers (a copy would have to
  // wait for the data). A loop iteration holds an even number of units:
  // one batch when TT is even, two batches when TT == 1 — there the second
  // may lie past K, where every piece is zero in both operands and the
  // MFMAs add exact zeros.
  constexpr int BPI = TT == 1 ? 2 : 1;       // batches per iteration
  const int NB = DTX_CDIV(K, SK_BATCH);
  const short8v z8 = {0, 0, 0, 0, 0, 0, 0, 0};
  short8v wbuf[2][SK_STEPS];
  sk_load(wbuf[0], wb, wr[0], wid * SK_BATCH, h, K);
  for (int b = wid; b < NB; b += BPI * SK_NW) {   // wave-uniform trip count
#pragma unroll
    for (int i = 0; i < BPI; ++i) {
      const int kb = (b + i * SK_NW) * SK_BATCH;
      short8v xc[SK_STEPS];
      sk_load(xc, X, xr, kb, h, K);
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        const int u = (i * TT + t) & 1;      // this unit's buffer
        // the next unit's loads go out before this unit's MFMAs
        if (t + 1 < TT)
          sk_load(wbuf[u ^ 1], (EPI == 2 && t + 1 >= T) ? ub : wb, wr[t + 1],
                  kb, h, K);
        else
          sk_load(wbuf[u ^ 1], wb, wr[0], kb + SK_NW * SK_BATCH, h, K);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < SK_STEPS; ++s) {
          const bool kin = kb + s * 32 + h * 8 < K;   // piece in or out
          acc[t] = MFMA16(kin ? wbuf[u][s] : z8,
                          (kin && mrow) ? xc[s] : z8, acc[t]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  // D layout: col (batch row m) = lane & 15, row (weight row) = 4 * h + reg
#pragma unroll
  for (int t = 0; t < TT; ++t)
    *reinterpret_cast<float4v*>(&red[((wid * TT + t) * 64 + lane) * 4]) =
        acc[t];
  __syncthreads();
  for (int e = tid; e < T * 256; e += SK_NW * 64) {
    const int t = e >> 8;
    const int m = (e >> 4) & 15;
    const int nl = e & 15;                       // consecutive threads:
    const int src = ((nl >> 2) * 16 + m) * 4 + (nl & 3);   // consecutive n
    float v = 0.f, u = 0.f;
#pragma unroll
    for (int w = 0; w < SK_NW; ++w) {            // fixed wave order
      v += red[(w * TT + t) * 256 + src];
      if (EPI == 2) u += red[(w * TT + T + t) * 256 + src];
    }
    const long n = n0 + t * 16 + nl;
    if (m < M && n < N) {
      const long o = (long)m * N + n;
      if (EPI == 1) v += bf2f(G.aux[o]);
      if (EPI == 2) v = dtx_swiglu(bf2f(f2bf(v)), bf2f(f2bf(u)));
      G.y[o] = f2bf(v);
    }
  }
}

// ------------------------------------------------------------------ launch
// The one contract of the family, shared by the bindings and Python: what
// the kernels can take (1..16 rows, whole 16-byte pieces of K, 32-bit
// lane offsets) minus what they lose to the library at. Measured
// (profiles/README.md, "Skinny bf16 decode"): at N >= 16384 (an lm_head)
// the x re-read from L2 costs as much as the library's tiling above two
// rows, so those calls stay where they were.
bool skinny_supported(long M, long N, long K) {
  return M >= 1 && M <= 16 && N >= 1 && N <= (1L << 30) && K >= 8 &&
         K % 8 == 0 && K <= (1L << 24) && (N < 16384 || M <= 2);
}

template <int T, int EPI>
static void skinny_launch(const void* x, const void* const* w,
                          const void* const* aux, void* const* y,
                          const int* N, int nw, int M, int K,
                          hipStream_t st) {
  SkinnyArgs a;
  int blocks = 0;
  for (int i = 0; i < SK_MAXW; ++i) {
    const int j = i < nw ? i : 0;          // unused slots: never selected
    a.g[i].w = (const unsigned short*)w[j];
    a.g[i].aux = (const unsigned short*)(aux ? aux[j] : nullptr);
    a.g[i].y = (unsigned short*)y[j];
    a.g[i].N = N[j];
    a.g[i].blk0 = i < nw ? blocks : 0x7fffffff;
    if (i < nw) blocks += (int)DTX_CDIV((long)N[i], 16 * T);
  }
  skinny_gemm_kernel<T, EPI><<<blocks, SK_NW * 64, 0, st>>>(
      (const unsigned short*)x, a, M, K);
}

// Tiles per x fragment from the rows of the launch. The x re-read from L2
// is what a block pays per tile-batch, so T = 4 as soon as N leaves enough
// blocks for the chip (measured: 11008 rows run 28 us at T = 1 or 2, 24 us
// at T = 4; 4096 rows 12 us at T = 1, 21 us at T = 4).
static int skinny_tiles(long n) { return n >= 8192 ? 4 : 1; }

void launch_skinny_gemm(const void* x, const void* const* w,
                        const void* residual, void* const* y, const int* N,
                        int nw, int M, int K, hipStream_t st) {
  long total = 0;
  for (int i = 0; i < nw; ++i) total += N[i];
  const int T = skinny_tiles(total);
  const void* const* aux = residual ? &residual : nullptr;
#define SK_GO(TT_)                                                         \
  (residual ? skinny_launch<TT_, 1>(x, w, aux, y, N, nw, M, K, st)         \
            : skinny_launch<TT_, 0>(x, w, aux, y, N, nw, M, K, st))
  if (T == 4) SK_GO(4); else SK_GO(1);
#undef SK_GO
}

void launch_skinny_swiglu(const void* x, const void* wg, const void* wu,
                          void* y, int M, int N, int K, hipStream_t st) {
  // two weight tiles per output tile: T = 1 (measured at 11008 rows),
  // T = 2 from an lm_head's size up
  if (N >= 16384)
    skinny_launch<2, 2>(x, &wg, &wu, &y, &N, 1, M, K, st);
  else
    skinny_launch<1, 2>(x, &wg, &wu, &y, &N, 1, M, K, st);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
