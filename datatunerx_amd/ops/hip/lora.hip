// Fused LoRA low-rank path (the hand-written hot path the north star
// names: "fused LoRA A/B + base GEMM" — the base GEMM runs on hipBLASLt,
// these kernels fuse everything low-rank around it).
//
// Layouts (HF PEFT adapter contract): A [r,K], B [N,r].
//   contract:   t[M,r]  = X[M,K] @ W[r,K]^T     (r <= 16: streaming MFMA
//               16x16x32 kernel, one or two adapters per pass over X;
//               r > 16: 32x32x16 kernel over zero-padded 32-col r tiles.
//               Both split K across blocks: fp32 partials + reduce)
//   expand_add: Y[M,N] += s * T[M,r] @ W[N,r]^T (W^T register-resident
//               per column slice; fused in-place epilogue on Y; the dual
//               form adds two adapters' terms in one pass over Y)
//   wgrad:      dW[r,K] = s * T[M,r]^T @ X[M,K] (deterministic split-M
//               partials + reduce, no atomics)
// All skinny/memory-bound: the roofline is streaming X/Y at HBM rate.
// R is a compile-time bound so accumulators stay in VGPRs (guide §5.4
// rule 20).
#include "dtx_mfma.h"
#include "dtx_launch.h"

// x (o mask) rounded to bf16, the operand every LoRA kernel contracts
// MODE 1: bf16 mask fragment; MODE 2: fp32 mask values from the RNG
__device__ __forceinline__ short8v lora_mask_bf16(short8v xf, short8v mf) {
  unsigned* xu = reinterpret_cast<unsigned*>(&xf);
#pragma unroll
  for (int e = 0; e < 8; e += 2) {
    float p0 = bf2f((unsigned short)xf[e]) * bf2f((unsigned short)mf[e]);
    float p1 = bf2f((unsigned short)xf[e + 1]) *
               bf2f((unsigned short)mf[e + 1]);
    xu[e / 2] = dtx_cvt_pk_bf16(p0, p1);
  }
  return xf;
}

__device__ __forceinline__ short8v lora_mask_f32(short8v xf,
                                                 const float mv[8]) {
  unsigned* xu = reinterpret_cast<unsigned*>(&xf);
#pragma unroll
  for (int e = 0; e < 8; e += 2)
    xu[e / 2] = dtx_cvt_pk_bf16(bf2f((unsigned short)xf[e]) * mv[e],
                                bf2f((unsigned short)xf[e + 1]) * mv[e + 1]);
  return xf;
}

// ------------------------------------------------------- contract, r <= 16
// Streaming plan. A block owns one LC_SPAN-wide k-slice (blockIdx.y) and
// stages that slice of the adapter(s) in LDS ONCE; its four waves then
// walk 16-row m-tiles of X (grid-stride), each tile one chain of
// 16x16x32 MFMAs with the accumulator in registers over the whole slice
// and a single store at the end (to the output when K fits one slice,
// else to this slice's fp32 partial plane, summed by reduce_partials).
//
// X is the MFMA A operand: lane l holds row (l & 15), k = 8*(l >> 4)+j,
// so one wave load is 16 rows x 64 contiguous bytes, and two consecutive
// k-steps finish each 128-byte line. LC_UNR independent 16-byte loads
// are in flight per lane before the first MFMA of a batch. All loads are
// unconditional (rows and k clamped, the out-of-range k zeroed by a
// select), so the compiler can count them (docs/kernels.md, "The
// waitcnt trap").
//
// B operand: lane reads the LDS row (l & 15) & (RP-1); output columns
// >= r are never stored, so those lanes may multiply anything finite or
// not — a column of D depends on its own column of B only. LDS rows
// r..RP-1 repeat row r-1 for the same reason; k >= K is staged as zero.
//
// NA = 2 contracts the same X tile against two adapters with two
// dropout seeds: each output sees exactly the operations of the NA = 1
// kernel (same slices, same MFMA chain), so it is bit-identical.
// MODE: 0 = no mask, 1 = bf16 mask tensor (NA = 1), 2 = in-kernel RNG
#define LC_SPAN 1024
#define LC_LDW (LC_SPAN + 8)       // +16 B: rows land on distinct banks
#define LC_UNR 8

template <int RP, int MODE, int NA>
__global__ __launch_bounds__(DTX_BLOCK)
void lora_contract_stream_kernel(const unsigned short* __restrict__ X,
                                 const unsigned short* __restrict__ W0,
                                 const unsigned short* __restrict__ W1,
                                 const unsigned short* __restrict__ Mk,
                                 float* __restrict__ dst,
                                 long M, int K, int r,
                                 unsigned long long seed0,
                                 unsigned long long seed1, unsigned thr16,
                                 float inv_keep) {
  __shared__ __attribute__((aligned(16)))
  unsigned short wl[NA * RP * LC_LDW];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int n = lane & 15;
  const int g = lane >> 4;
  const int k0 = blockIdx.y * LC_SPAN;
  const int klen = min(LC_SPAN, K - k0);     // > 0, multiple of 8

  for (int idx = threadIdx.x; idx < NA * RP * (LC_SPAN / 8);
       idx += DTX_BLOCK) {
    const int c = idx % (LC_SPAN / 8);
    const int row = (idx / (LC_SPAN / 8)) % RP;
    const int a = idx / (RP * (LC_SPAN / 8));
    const unsigned short* W = (NA == 2 && a) ? W1 : W0;
    short8v w8 = *reinterpret_cast<const short8v*>(
        &W[(long)min(row, r - 1) * K + k0 + min(c * 8, klen - 8)]);
    if (c * 8 >= klen) w8 = short8v{0, 0, 0, 0, 0, 0, 0, 0};
    *reinterpret_cast<short8v*>(&wl[(a * RP + row) * LC_LDW + c * 8]) = w8;
  }
  __syncthreads();

  const int nsteps = DTX_CDIV(klen, 32);
  const unsigned short* wrow = &wl[(n & (RP - 1)) * LC_LDW + g * 8];
  for (long mt = (long)blockIdx.x * 4 + wid; mt * 16 < M;
       mt += (long)gridDim.x * 4) {
    const long xrow = min(mt * 16 + n, M - 1);
    const long rbase = xrow * K + k0;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < nsteps; s0 += LC_UNR) {
      short8v xf[LC_UNR], mf[LC_UNR];
#pragma unroll
      for (int u = 0; u < LC_UNR; ++u) {
        const int kc = min((s0 + u) * 32 + g * 8, klen - 8);
        xf[u] = *reinterpret_cast<const short8v*>(X + rbase + kc);
        if (MODE == 1)
          mf[u] = *reinterpret_cast<const short8v*>(Mk + rbase + kc);
      }
#pragma unroll
      for (int u = 0; u < LC_UNR; ++u) {
        const int kk = (s0 + u) * 32 + g * 8;   // <= LC_SPAN - 8: in wl
        const bool live = kk < klen;
        const int kc = min(kk, klen - 8);
        short8v x0 = xf[u], x1 = xf[u];
        if (MODE == 1) {
          x0 = lora_mask_bf16(xf[u], mf[u]);
        } else if (MODE == 2) {
          const unsigned long long ctr = dtx_dropout_ctr(rbase + kc);
          float mv[8];
          dtx_dropout8_ctr(seed0, ctr, thr16, inv_keep, mv);
          x0 = lora_mask_f32(xf[u], mv);
          if (NA == 2) {
            dtx_dropout8_ctr(seed1, ctr, thr16, inv_keep, mv);
            x1 = lora_mask_f32(xf[u], mv);
          }
        }
        const short8v z8 = {0, 0, 0, 0, 0, 0, 0, 0};
        x0 = live ? x0 : z8;
        acc0 = MFMA16(x0, *reinterpret_cast<const short8v*>(
                              wrow + (s0 + u) * 32), acc0);
        if (NA == 2) {
          x1 = live ? x1 : z8;
          acc1 = MFMA16(x1, *reinterpret_cast<const short8v*>(
                                wrow + RP * LC_LDW + (s0 + u) * 32), acc1);
        }
      }
    }
    // C-layout: col = r-index n, row = 4*g + q
    if (n < r) {
      float* p0 = dst + ((long)blockIdx.y * NA) * M * r;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const long m = mt * 16 + g * 4 + q;
        if (m < M) {
          p0[m * r + n] = acc0[q];
          if (NA == 2) p0[(M + m) * r + n] = acc1[q];
        }
      }
    }
  }
}

// -------------------------------------------------------- contract, r > 16
// One wave = one 32-row m-tile x 32-col r-tile (cols >= r zero-padded).
// A-frag: lane streams X[mw+l31][kc*16 + hi*8 + j] straight from HBM
// (each row read once; 8 kc loads/lane = 128 contiguous bytes).
// B-frag: lane reads the LDS copy of W at row l31 (zero rows >= r).
// Split-K across blockIdx.y; fp32 partials reduced by reduce_partials.
// MODE: 0 = no mask, 1 = bf16 mask tensor, 2 = in-kernel RNG dropout
template <int MODE>
__global__ __launch_bounds__(DTX_BLOCK)
void lora_contract_kernel(const unsigned short* __restrict__ X,
                          const unsigned short* __restrict__ W,
                          const unsigned short* __restrict__ Mk,
                          float* __restrict__ part,
                          long M, int K, int r, int kspan,
                          unsigned long long seed, unsigned thr16,
                          float inv_keep) {
  __shared__ unsigned short wlds[32][1024 + 8];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int l31 = lane & 31;
  const int hi = lane >> 5;
  const int k0 = blockIdx.y * kspan;
  const int kend = min(K, k0 + kspan);

  float* pout = part + (long)blockIdx.y * M * r;

  for (int kc0 = k0; kc0 < kend; kc0 += 1024) {
    const int kc_n = min(1024, kend - kc0);
    for (int rt = 0; rt < r; rt += 32) {
      // stage 32 W rows (zero-padded) for this (r-tile, k-chunk)
      for (int idx = threadIdx.x; idx < 32 * (1024 / 8); idx += DTX_BLOCK) {
        const int row = idx / 128, g = idx % 128;
        short8v w8 = {0, 0, 0, 0, 0, 0, 0, 0};
        if (rt + row < r && g * 8 < kc_n)
          w8 = *reinterpret_cast<const short8v*>(
              &W[(long)(rt + row) * K + kc0 + g * 8]);
        *reinterpret_cast<short8v*>(&wlds[row][g * 8]) = w8;
      }
      __syncthreads();

      for (long mw = (long)(blockIdx.x * 4 + wid) * 32; mw < M;
           mw += (long)gridDim.x * 4 * 32) {
        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
        const long xrow = mw + l31;
        const long rbase = xrow * K + kc0;
        const unsigned short* xp = xrow < M ? X + rbase : X;
        const unsigned short* mp =
            (MODE == 1 && xrow < M) ? Mk + rbase : nullptr;
        for (int kc = 0; kc < kc_n; kc += 16) {
          short8v xf = xrow < M
              ? *reinterpret_cast<const short8v*>(xp + kc + hi * 8)
              : short8v{0, 0, 0, 0, 0, 0, 0, 0};
          // The operations of lora_mask_bf16 / lora_mask_f32, kept
          // written out: through the helpers this kernel takes two more
          // VGPRs (MODE 1: 62 -> 64; MODE 2: 64 -> 66, one wave per
          // SIMD less).
          if (MODE == 1 && mp) {
            short8v mf = *reinterpret_cast<const short8v*>(
                mp + kc + hi * 8);
            unsigned* xu = reinterpret_cast<unsigned*>(&xf);
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
              float p0 = bf2f((unsigned short)xf[e]) *
                         bf2f((unsigned short)mf[e]);
              float p1 = bf2f((unsigned short)xf[e + 1]) *
                         bf2f((unsigned short)mf[e + 1]);
              xu[e / 2] = dtx_cvt_pk_bf16(p0, p1);
            }
          } else if (MODE == 2 && xrow < M) {
            float mv[8];
            dtx_dropout8(seed, rbase + kc + hi * 8, thr16, inv_keep, mv);
            unsigned* xu = reinterpret_cast<unsigned*>(&xf);
#pragma unroll
            for (int e = 0; e < 8; e += 2)
              xu[e / 2] = dtx_cvt_pk_bf16(
                  bf2f((unsigned short)xf[e]) * mv[e],
                  bf2f((unsigned short)xf[e + 1]) * mv[e + 1]);
          }
          short8v wf = *reinterpret_cast<const short8v*>(
              &wlds[l31][kc + hi * 8]);
          acc = MFMA32(xf, wf, acc);
        }
        // C-layout: col = r-index = rt + l31, row m = crow(q,hi)
        if (rt + l31 < r) {
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const long m = mw + crow(q, hi);
            if (m < M) {
              if (kc0 == k0)
                pout[m * r + rt + l31] = acc[q];
              else
                pout[m * r + rt + l31] += acc[q];
            }
          }
        }
      }
      __syncthreads();
    }
  }
}

// -------------------------------------------------------------- expand_add
// Y[M,N] += (mask o) s * T[M,r] @ WT[r,N].  WT is the adapter in [r,N]
// (lora_A as it is; lora_B transposed by the caller, once per forward:
// 64 KB, L1/L2-resident), so every access here is a coalesced 16-byte
// load — no LDS staging pass.
// j blocked by 8 so register pressure is independent of r.
template <bool MASKED>
__global__ __launch_bounds__(DTX_BLOCK)
void lora_expand_add_kernel(unsigned short* __restrict__ Y,
                            const float* __restrict__ T,
                            const unsigned short* __restrict__ WT,
                            const unsigned short* __restrict__ Mk,
                            long M, int N, int r, float s) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  for (long m = blockIdx.x * 4 + wid; m < M; m += (long)gridDim.x * 4) {
    const float* tr = T + m * r;
    unsigned short* yr = Y + m * N;
    const unsigned short* mr = MASKED ? Mk + m * N : nullptr;
    for (int n = lane * 8; n < N; n += WAVE * 16) {
      const int n2 = n + WAVE * 8;
      const bool l2 = n2 < N;
      float a0[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      float a1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int jb = 0; jb < r; jb += 8) {
        float tv[8];
#pragma unroll
        for (int t = 0; t < 8; ++t)
          tv[t] = (jb + t < r) ? s * tr[jb + t] : 0.f;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          if (jb + t < r) {
            const unsigned short* wrow = WT + (long)(jb + t) * N;
            float w0[8], w1[8];
            load_bf16x8(wrow + n, w0);
            if (l2) load_bf16x8(wrow + n2, w1);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              a0[i] += tv[t] * w0[i];
              if (l2) a1[i] += tv[t] * w1[i];
            }
          }
        }
      }
      float y0[8], y1[8];
      load_bf16x8(yr + n, y0);
      if (l2) load_bf16x8(yr + n2, y1);
      if (MASKED) {
        float m0[8], m1[8];
        load_bf16x8(mr + n, m0);
        if (l2) load_bf16x8(mr + n2, m1);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          y0[i] += m0[i] * a0[i];
          if (l2) y1[i] += m1[i] * a1[i];
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          y0[i] += a0[i];
          if (l2) y1[i] += a1[i];
        }
      }
      store_bf16x8(yr + n, y0);
      if (l2) store_bf16x8(yr + n2, y1);
    }
  }
}

// ------------------------------------------------------------------ wgrad
// part[ms][j][K] = s * sum_{m in split ms} T[m,j] * X[m,k]
// (k-span 2048/block keeps X re-reads at ceil(K/2048); the partials are
// streamed back by the vectorized reduce_partials kernel)
template <int RCH, int MODE>
__global__ __launch_bounds__(DTX_BLOCK)
void lora_wgrad_kernel(const float* __restrict__ T,
                       const unsigned short* __restrict__ X,
                       const unsigned short* __restrict__ Mk,
                       float* __restrict__ part,
                       long M, int K, int r, int j0, int splitm, float s,
                       unsigned long long seed, unsigned thr16,
                       float inv_keep) {
  const int col = blockIdx.x * 2048 + threadIdx.x * 8;
  const int ms = blockIdx.y;
  if (col >= K) return;
  float acc[RCH][8];
#pragma unroll
  for (int j = 0; j < RCH; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[j][i] = 0.f;
  const long m_begin = (M * ms) / splitm;
  const long m_end = (M * (ms + 1)) / splitm;
  for (long m = m_begin; m < m_end; ++m) {
    float xv[8];
    load_bf16x8(X + m * K + col, xv);
    if (MODE >= 1) {
      float mv[8];
      if (MODE == 1) load_bf16x8(Mk + m * K + col, mv);
      else dtx_dropout8(seed, m * K + col, thr16, inv_keep, mv);
#pragma unroll
      for (int i = 0; i < 8; i += 2) {       // match bf16 x*mask numerics
        unsigned pk = dtx_cvt_pk_bf16(xv[i] * mv[i], xv[i + 1] * mv[i + 1]);
        xv[i] = bf2f((unsigned short)(pk & 0xffffu));
        xv[i + 1] = bf2f((unsigned short)(pk >> 16));
      }
    }
    const float* tr = T + m * r + j0;
#pragma unroll
    for (int j = 0; j < RCH; ++j) {
      if (j0 + j < r) {
        float t = tr[j];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[j][i] += t * xv[i];
      }
    }
  }
  float* pb = part + ((long)ms * r) * K;
#pragma unroll
  for (int j = 0; j < RCH; ++j) {
    if (j0 + j < r) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        pb[(long)(j0 + j) * K + col + i] = s * acc[j][i];
    }
  }
}

// Register-hoisted expand_add for the common small ranks (r <= 16):
// each block owns a 2048-column slice of Y and a row range; the WT
// slice lives in REGISTERS for the whole row loop, so the only memory
// traffic per row is T (lane-uniform 4B*r), Y in/out and the mask --
// the v1 kernel re-read WT from L2 for every row (64 KB/row/wave) and
// sat at ~2.8 TB/s; this one runs at the streaming roofline.
template <int RCH, int MODE>
__global__ __launch_bounds__(DTX_BLOCK)
void lora_expand_add_kernel2(unsigned short* __restrict__ Y,
                             const float* __restrict__ T,
                             const unsigned short* __restrict__ WT,
                             const unsigned short* __restrict__ Mk,
                             long M, int N, int r, float s, int rowsplit,
                             unsigned long long seed, unsigned thr16,
                             float inv_keep) {
  const int col = blockIdx.x * 2048 + threadIdx.x * 8;
  if (col >= N) return;                      // N % 8 == 0 (checked host)
  float w[RCH][8];
#pragma unroll
  for (int j = 0; j < RCH; ++j) {
    if (j < r) {
      load_bf16x8(WT + (long)j * N + col, w[j]);
#pragma unroll
      for (int i = 0; i < 8; ++i) w[j][i] *= s;
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) w[j][i] = 0.f;
    }
  }
  const long m0 = (M * (long)blockIdx.y) / rowsplit;
  const long m1 = (M * (long)(blockIdx.y + 1)) / rowsplit;
  for (long m = m0; m < m1; ++m) {
    const float* tr = T + m * r;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < RCH; ++j) {
      if (j < r) {
        const float t = tr[j];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += t * w[j][i];
      }
    }
    unsigned short* yp = Y + m * N + col;
    float y[8];
    load_bf16x8(yp, y);
    if (MODE >= 1) {
      float mv[8];
      if (MODE == 1) load_bf16x8(Mk + m * N + col, mv);
      else dtx_dropout8(seed, m * N + col, thr16, inv_keep, mv);
#pragma unroll
      for (int i = 0; i < 8; ++i) y[i] += mv[i] * acc[i];
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) y[i] += acc[i];
    }
    store_bf16x8(yp, y);
  }
}

// ------------------------------------------------------- dual expand_add
// Y[M,N] += mask0 o (s * T0 @ A0) + mask1 o (s * T1 @ A1), A0/A1 in the
// [r,N] layout (native lora_A for the dx term of the backward): one
// read-modify-write of Y and one bf16 rounding for both adapters. Same
// register-hoisted structure as lora_expand_add_kernel2; a thread owns
// CW columns (8 for r <= 8; 4 for r <= 16 so the two hoisted adapter
// slices stay at 128 registers). Four rows of Y in flight per lane.
// MODE: 0 = no mask, 2 = in-kernel RNG (seed0 / seed1)
template <int CW>
__device__ __forceinline__ void ld_bf16(const unsigned short* p, float* o) {
  if (CW == 8) {
    load_bf16x8(p, o);
  } else {
    short4v v = *reinterpret_cast<const short4v*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = bf2f((unsigned short)v[i]);
  }
}

template <int RCH, int CW, int MODE>
__global__ __launch_bounds__(DTX_BLOCK, 2)
void lora_expand_add_dual_kernel(unsigned short* __restrict__ Y,
                                 const float* __restrict__ T0,
                                 const float* __restrict__ T1,
                                 const unsigned short* __restrict__ A0,
                                 const unsigned short* __restrict__ A1,
                                 long M, int N, int r, float s,
                                 int rowsplit, unsigned long long seed0,
                                 unsigned long long seed1, unsigned thr16,
                                 float inv_keep) {
  const int col = (blockIdx.x * DTX_BLOCK + threadIdx.x) * CW;
  if (col >= N) return;                      // N % 8 == 0 (checked host)
  float w0[RCH][CW], w1[RCH][CW];
#pragma unroll
  for (int j = 0; j < RCH; ++j) {
    if (j < r) {
      ld_bf16<CW>(A0 + (long)j * N + col, w0[j]);
      ld_bf16<CW>(A1 + (long)j * N + col, w1[j]);
#pragma unroll
      for (int i = 0; i < CW; ++i) { w0[j][i] *= s; w1[j][i] *= s; }
    } else {
#pragma unroll
      for (int i = 0; i < CW; ++i) w0[j][i] = w1[j][i] = 0.f;
    }
  }
  const long m0 = (M * (long)blockIdx.y) / rowsplit;
  const long m1 = (M * (long)(blockIdx.y + 1)) / rowsplit;
  for (long mb = m0; mb < m1; mb += 4) {
    float y[4][CW];
#pragma unroll
    for (int u = 0; u < 4; ++u)            // rows clamped: loads unconditional
      ld_bf16<CW>(Y + min(mb + u, m1 - 1) * N + col, y[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long m = min(mb + u, m1 - 1);
      const float* t0 = T0 + m * r;
      const float* t1 = T1 + m * r;
      float a0[CW], a1[CW];
#pragma unroll
      for (int i = 0; i < CW; ++i) a0[i] = a1[i] = 0.f;
#pragma unroll
      for (int j = 0; j < RCH; ++j) {
        if (j < r) {
          const float p = t0[j], q = t1[j];
#pragma unroll
          for (int i = 0; i < CW; ++i) {
            a0[i] += p * w0[j][i];
            a1[i] += q * w1[j][i];
          }
        }
      }
      if (MODE == 2) {
        // one RNG group covers 4 elements, so a CW = 4 thread draws
        // exactly its own group
        const unsigned long long ctr = dtx_dropout_ctr(m * N + col);
        float mv0[8], mv1[8];
        if (CW == 8) {
          dtx_dropout8_ctr(seed0, ctr, thr16, inv_keep, mv0);
          dtx_dropout8_ctr(seed1, ctr, thr16, inv_keep, mv1);
        } else {
          dtx_dropout4_z(seed0 + ctr, thr16, inv_keep, mv0);
          dtx_dropout4_z(seed1 + ctr, thr16, inv_keep, mv1);
        }
#pragma unroll
        for (int i = 0; i < CW; ++i)
          y[u][i] += mv0[i] * a0[i] + mv1[i] * a1[i];
      } else {
#pragma unroll
        for (int i = 0; i < CW; ++i) y[u][i] += a0[i] + a1[i];
      }
      if (mb + u < m1) {
        unsigned short* yp = Y + m * N + col;
        if (CW == 8) {
          store_bf16x8(yp, y[u]);
        } else {
          short4v v;
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = (short)f2bf(y[u][i]);
          *reinterpret_cast<short4v*>(yp) = v;
        }
      }
    }
  }
}

// Standalone mask materializer (tests + the r>16 fallback path): the
// EXACT bits the fused MODE==2 kernels consume, as a bf16 tensor.
__global__ __launch_bounds__(DTX_BLOCK)
void dropout_mask_kernel(unsigned short* __restrict__ Mk, long n8,
                         unsigned long long seed, unsigned thr16,
                         float inv_keep) {
  long idx = (long)blockIdx.x * DTX_BLOCK + threadIdx.x;
  long stride = (long)gridDim.x * DTX_BLOCK;
  for (; idx < n8; idx += stride) {
    float mv[8];
    dtx_dropout8(seed, idx * 8, thr16, inv_keep, mv);
    store_bf16x8(Mk + idx * 8, mv);
  }
}

static void dropout_spec(float keep, unsigned* thr16, float* inv_keep) {
  double t = (double)keep * 65536.0 + 0.5;
  *thr16 = t >= 65536.0 ? 65536u : (unsigned)t;
  // the mask VALUE is the bf16-rounded 1/keep (identical numerics to a
  // materialized bf16 mask tensor)
  union { float f; unsigned u; } x;
  x.f = 1.0f / keep;
  unsigned r = 0x7fffu + ((x.u >> 16) & 1u);
  x.u = ((x.u + r) >> 16) << 16;
  *inv_keep = x.f;
}

// The kernels' MODE template argument and the RNG constants, from what a
// launcher is given: 1 = bf16 mask tensor Mk (it wins over keep),
// 2 = in-kernel RNG (keep < 1 and no Mk), 0 = no dropout.
struct LoraDropout {
  int mode;
  unsigned thr16 = 0;
  float inv_keep = 1.f;
  LoraDropout(const void* Mk, float keep)
      : mode(Mk ? 1 : keep < 1.f ? 2 : 0) {
    if (mode == 2) dropout_spec(keep, &thr16, &inv_keep);
  }
};
// LAUNCH(MODE) with d.mode as the compile-time MODE
#define LORA_MODE_SWITCH(d, LAUNCH)                                       \
  do {                                                                    \
    if ((d).mode == 1) LAUNCH(1);                                         \
    else if ((d).mode == 2) LAUNCH(2);                                    \
    else LAUNCH(0);                                                       \
  } while (0)

// Shapes lora_expand_add_kernel2 takes; the v1 kernel that takes the
// rest has no RNG mode (the ops layer materializes the mask for it).
bool lora_expand_rng_ok(long M, int N, int r) {
  return r <= 16 && N % 8 == 0 && M >= 64;
}

// ------------------------------------------------------------- launchers
void launch_dropout_mask(void* Mk, long n, unsigned long long seed,
                         float keep, hipStream_t s) {
  unsigned thr16; float ik;
  dropout_spec(keep, &thr16, &ik);
  long g = DTX_CDIV(n / 8, DTX_BLOCK);
  int grid = (int)(g < 2048 ? (g < 1 ? 1 : g) : 2048);
  dropout_mask_kernel<<<grid, DTX_BLOCK, 0, s>>>(
      (unsigned short*)Mk, n / 8, seed, thr16, ik);
}

// split plan: spans are MULTIPLES OF 1024 elements so every staged
// 16-byte load stays aligned (K=5120 used to produce a 1707-element
// span -> misaligned b128 loads -> GPU memory fault on the 13B shapes).
static int lora_contract_kspan(int K) {
  int units = DTX_CDIV(K, 1024);
  int nsplit = units < 4 ? units : 4;
  return DTX_CDIV(units, nsplit) * 1024;
}

// Contract plan, a pure function of (M, K, r): the number of k-slices
// (= fp32 partial planes; 1 means the kernel writes the output itself).
//   r <= 16  streaming kernel: one LC_SPAN slice per block whatever M
//            is. Slices, not rows, are what lets a block stage its
//            adapter slice once and still leave LDS for 4 blocks per
//            CU; the partials are M*r*4 bytes per slice, under 2 % of
//            the X bytes even at K = 11008.
//   r > 16   32x32x16 kernel: up to 4 slices to fill the chip at small
//            M; at M >= 32K rows the m-tiles alone fill it.
int lora_contract_ksplit(int K, long M, int r) {
  if (r <= 16)
    return DTX_CDIV(K, LC_SPAN);
  if (M >= (128L * 256))
    return 1;
  return DTX_CDIV(K, lora_contract_kspan(K));
}

// na adapters (1 or 2) against one X: out [na][M][r], part
// [nsplit][na][M][r]. ~1024 blocks = 4 per CU; a block grid-strides over
// m so the staged slice is reused.
static void launch_contract_stream(const void* X, const void* W0,
                                   const void* W1, const void* Mk,
                                   float* part, float* out, long M, int K,
                                   int r, int na, unsigned long long seed0,
                                   unsigned long long seed1, float keep,
                                   hipStream_t s) {
  const int nsplit = DTX_CDIV(K, LC_SPAN);
  long gx = DTX_CDIV(M, 64);
  const long cap = 1024 / nsplit > 0 ? 1024 / nsplit : 1;
  if (gx > cap) gx = cap;
  if (gx < 1) gx = 1;
  dim3 grid((int)gx, nsplit);
  float* dst = nsplit > 1 ? part : out;
  const LoraDropout d(Mk, keep);
#define STREAM(RP, MODE, NA)                                              \
  lora_contract_stream_kernel<RP, MODE, NA><<<grid, DTX_BLOCK, 0, s>>>(   \
      (const unsigned short*)X, (const unsigned short*)W0,                \
      (const unsigned short*)W1, (const unsigned short*)Mk, dst, M, K, r, \
      seed0, seed1, d.thr16, d.inv_keep)
#define STREAM1(MODE)                                                     \
  do { if (r <= 8) STREAM(8, MODE, 1); else STREAM(16, MODE, 1); } while (0)
#define STREAM2(MODE)                                                     \
  do { if (r <= 8) STREAM(8, MODE, 2); else STREAM(16, MODE, 2); } while (0)
  if (na == 1) LORA_MODE_SWITCH(d, STREAM1);
  else if (d.mode == 2) STREAM2(2);        // the dual form takes no mask
  else STREAM2(0);
#undef STREAM2
#undef STREAM1
#undef STREAM
  if (nsplit > 1)
    launch_reduce_partials(part, out, nsplit, (long)na * M * r, s);
}

void launch_lora_contract2(const void* X, const void* W0, const void* W1,
                           float* part, float* out, long M, int K, int r,
                           unsigned long long seed0,
                           unsigned long long seed1, float keep,
                           hipStream_t s) {
  launch_contract_stream(X, W0, W1, nullptr, part, out, M, K, r, 2, seed0,
                         seed1, keep, s);
}

void launch_lora_contract(const void* X, const void* W, const void* Mk,
                          float* part, float* out, long M, int K, int r,
                          unsigned long long seed, float keep,
                          hipStream_t s) {
  if (r <= 16) {
    launch_contract_stream(X, W, W, Mk, part, out, M, K, r, 1, seed, seed,
                           keep, s);
    return;
  }
  const int nsplit = lora_contract_ksplit(K, M, r);
  const int kspan = nsplit == 1 ? DTX_CDIV(K, 1024) * 1024
                                : lora_contract_kspan(K);
  long gw = DTX_CDIV(M, 128);
  dim3 grid((int)(gw < 128 ? (gw < 1 ? 1 : gw) : 128), nsplit);
  float* dst = nsplit > 1 ? part : out;
  const LoraDropout d(Mk, keep);
#define CONTRACT(MODE)                                                    \
  lora_contract_kernel<MODE><<<grid, DTX_BLOCK, 0, s>>>(                  \
      (const unsigned short*)X, (const unsigned short*)W,                 \
      (const unsigned short*)Mk, dst, M, K, r, kspan, seed, d.thr16,      \
      d.inv_keep)
  LORA_MODE_SWITCH(d, CONTRACT);
#undef CONTRACT
  if (nsplit > 1)
    launch_reduce_partials(part, out, nsplit, M * r, s);
}

void launch_lora_expand_add(void* Y, const float* T, const void* WT,
                            const void* Mk, long M, int N, int r,
                            float scale, unsigned long long seed,
                            float keep, hipStream_t s) {
  if (lora_expand_rng_ok(M, N, r)) {
    const LoraDropout d(Mk, keep);
    const int gx = DTX_CDIV(N, 2048);
    int rowsplit = 1024 / gx;
    if (rowsplit > M) rowsplit = (int)M;
    if (rowsplit < 1) rowsplit = 1;
    dim3 grid(gx, rowsplit);
#define EX2(RC, MODE)                                                     \
    lora_expand_add_kernel2<RC, MODE><<<grid, DTX_BLOCK, 0, s>>>(         \
        (unsigned short*)Y, T, (const unsigned short*)WT,                 \
        (const unsigned short*)Mk, M, N, r, scale, rowsplit, seed,        \
        d.thr16, d.inv_keep)
#define EX2R(MODE)                                                        \
    do {                                                                  \
      if (r <= 4) EX2(4, MODE);                                           \
      else if (r <= 8) EX2(8, MODE);                                      \
      else EX2(16, MODE);                                                 \
    } while (0)
    LORA_MODE_SWITCH(d, EX2R);
#undef EX2R
#undef EX2
    return;
  }
  // v1 fallback (r > 16 or tiny M) has no RNG mode: the binding refuses
  // it and ops.lora_expand_add_t materializes the mask for those shapes
  long gw = DTX_CDIV(M, 4);
  int grid = (int)(gw < 2048 ? (gw < 1 ? 1 : gw) : 2048);
  if (Mk) {
    lora_expand_add_kernel<true><<<grid, DTX_BLOCK, 0, s>>>(
        (unsigned short*)Y, T, (const unsigned short*)WT,
        (const unsigned short*)Mk, M, N, r, scale);
  } else {
    lora_expand_add_kernel<false><<<grid, DTX_BLOCK, 0, s>>>(
        (unsigned short*)Y, T, (const unsigned short*)WT, nullptr, M, N,
        r, scale);
  }
}

int lora_wgrad_splitm(int K, int r, long M) {
  int kblocks = DTX_CDIV(K, 2048);
  // target ~1024 blocks (4/CU -> 4 waves/SIMD); the old 512/cap-128
  // plan put ONE wave per SIMD on K=4096 and left 3.5x bandwidth idle
  int sm = 2048 / kblocks;
  // keep the fp32 partial buffer under ~256 MB
  long cap_mem = (256L << 20) / ((long)r * K * 4);
  if (sm > cap_mem) sm = (int)cap_mem;
  if (sm > M) sm = (int)M;
  return sm < 1 ? 1 : (sm > 512 ? 512 : sm);
}

void launch_lora_wgrad(const float* T, const void* X, const void* Mk,
                       float* part, float* out, long M, int K, int r,
                       float s, unsigned long long seed, float keep,
                       hipStream_t st) {
  const int splitm = lora_wgrad_splitm(K, r, M);
  dim3 grid(DTX_CDIV(K, 2048), splitm);
  const LoraDropout d(Mk, keep);
  for (int j0 = 0; j0 < r; j0 += 16) {
    int rch = r - j0;
#define WG(RC, MODE)                                                      \
    lora_wgrad_kernel<RC, MODE><<<grid, DTX_BLOCK, 0, st>>>(              \
        T, (const unsigned short*)X, (const unsigned short*)Mk, part,     \
        M, K, r, j0, splitm, s, seed, d.thr16, d.inv_keep)
#define WGR(MODE)                                                         \
    do {                                                                  \
      if (rch <= 4) WG(4, MODE);                                          \
      else if (rch <= 8) WG(8, MODE);                                     \
      else WG(16, MODE);                                                  \
    } while (0)
    LORA_MODE_SWITCH(d, WGR);
#undef WGR
#undef WG
  }
  launch_reduce_partials(part, out, splitm, (long)r * K, st);
}

// Dual expand-add, A0/A1 [r,N]; r <= 16 and N % 8 == 0 (checked by the
// binding). ~1024 blocks like the single kernel.
void launch_lora_expand_add_dual(void* Y, const float* T0, const float* T1,
                                 const void* A0, const void* A1, long M,
                                 int N, int r, float scale,
                                 unsigned long long seed0,
                                 unsigned long long seed1, float keep,
                                 hipStream_t s) {
  const LoraDropout d(nullptr, keep);
  const bool rng = d.mode == 2;
  const int cw = r <= 8 ? 8 : 4;
  const int gx = DTX_CDIV(N, DTX_BLOCK * cw);
  int rowsplit = 1024 / gx;
  if (rowsplit > M) rowsplit = (int)M;
  if (rowsplit < 1) rowsplit = 1;
  dim3 grid(gx, rowsplit);
#define EXD(RC, CW, MODE)                                                 \
  lora_expand_add_dual_kernel<RC, CW, MODE><<<grid, DTX_BLOCK, 0, s>>>(   \
      (unsigned short*)Y, T0, T1, (const unsigned short*)A0,              \
      (const unsigned short*)A1, M, N, r, scale, rowsplit, seed0, seed1,  \
      d.thr16, d.inv_keep)
  if (r <= 4) { if (rng) EXD(4, 8, 2); else EXD(4, 8, 0); }
  else if (r <= 8) { if (rng) EXD(8, 8, 2); else EXD(8, 8, 0); }
  else { if (rng) EXD(16, 4, 2); else EXD(16, 4, 0); }
#undef EXD
}
