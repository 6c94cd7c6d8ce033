// Fused LoRA low-rank path (the hand-written hot path the north star
// names: "fused LoRA A/B + base GEMM" — the base GEMM runs on hipBLASLt,
// these kernels fuse everything low-rank around it).
//
// Layouts (HF PEFT adapter contract): A [r,K], B [N,r].
//   contract:   t[M,r]  = X[M,K] @ W[r,K]^T     (MFMA 32x32x16 over a
//               zero-padded 32-col r tile; split-K partials + reduce)
//   expand_add: Y[M,N] += s * T[M,r] @ W[N,r]^T (W^T LDS-resident; one
//               wave per row, 2-chunk ILP; fused in-place epilogue on Y)
//   wgrad:      dW[r,K] = s * T[M,r]^T @ X[M,K] (deterministic split-M
//               partials + reduce, no atomics)
// All skinny/memory-bound: the roofline is streaming X/Y at HBM rate.
// R is a compile-time bound so accumulators stay in VGPRs (guide §5.4
// rule 20).
#include "dtx_mfma.h"

// ---------------------------------------------------------------- contract
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
// Y[M,N] += (mask o) s * T[M,r] @ WT[r,N].  WT is the PRE-TRANSPOSED
// adapter (binding does w.t().contiguous(): 64 KB, L1/L2-resident), so
// every access here is a coalesced 16-byte load — no LDS staging pass.
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

// ------------------------------------------------------------- launchers
void launch_reduce_partials(const float* part, float* out, int P, long L,
                            hipStream_t s);

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

int lora_contract_ksplit(int K, long M) {
  // K-split exists to FILL the chip when M alone cannot (grid.x tops
  // out at 128 four-wave blocks). At M >= 32K rows the m-tiles already
  // saturate every CU, and splitting only adds the fp32 partials +
  // reduce pass — skip it (mb64 shapes: M = 65536).
  if (M >= (128L * 256))
    return 1;
  return DTX_CDIV(K, lora_contract_kspan(K));
}

void launch_lora_contract(const void* X, const void* W, const void* Mk,
                          float* part, float* out, long M, int K, int r,
                          unsigned long long seed, float keep,
                          hipStream_t s) {
  const int nsplit = lora_contract_ksplit(K, M);
  const int kspan = nsplit == 1 ? DTX_CDIV(K, 1024) * 1024
                                : lora_contract_kspan(K);
  long gw = DTX_CDIV(M, 128);
  dim3 grid((int)(gw < 128 ? (gw < 1 ? 1 : gw) : 128), nsplit);
  float* dst = nsplit > 1 ? part : out;
  unsigned thr16 = 0; float ik = 1.f;
  if (!Mk && keep < 1.f) dropout_spec(keep, &thr16, &ik);
#define CONTRACT(MODE)                                                    \
  lora_contract_kernel<MODE><<<grid, DTX_BLOCK, 0, s>>>(                  \
      (const unsigned short*)X, (const unsigned short*)W,                 \
      (const unsigned short*)Mk, dst, M, K, r, kspan, seed, thr16, ik)
  if (Mk) CONTRACT(1);
  else if (keep < 1.f) CONTRACT(2);
  else CONTRACT(0);
#undef CONTRACT
  if (nsplit > 1)
    launch_reduce_partials(part, out, nsplit, M * r, s);
}

void launch_lora_expand_add(void* Y, const float* T, const void* WT,
                            const void* Mk, long M, int N, int r,
                            float scale, unsigned long long seed,
                            float keep, hipStream_t s) {
  const bool rng = !Mk && keep < 1.f;
  unsigned thr16 = 0; float ik = 1.f;
  if (rng) dropout_spec(keep, &thr16, &ik);
  if (r <= 16 && N % 8 == 0 && M >= 64) {
    const int gx = DTX_CDIV(N, 2048);
    int rowsplit = 1024 / gx;
    if (rowsplit > M) rowsplit = (int)M;
    if (rowsplit < 1) rowsplit = 1;
    dim3 grid(gx, rowsplit);
#define EX2(RC, MODE)                                                     \
    lora_expand_add_kernel2<RC, MODE><<<grid, DTX_BLOCK, 0, s>>>(         \
        (unsigned short*)Y, T, (const unsigned short*)WT,                 \
        (const unsigned short*)Mk, M, N, r, scale, rowsplit, seed,        \
        thr16, ik)
#define EX2M(RC)                                                          \
    do {                                                                  \
      if (Mk) EX2(RC, 1);                                                 \
      else if (rng) EX2(RC, 2);                                           \
      else EX2(RC, 0);                                                    \
    } while (0)
    if (r <= 4) EX2M(4);
    else if (r <= 8) EX2M(8);
    else EX2M(16);
#undef EX2M
#undef EX2
    return;
  }
  // v1 fallback (r > 16 or tiny M) has no RNG mode: callers materialize
  // the mask for those shapes (ops dispatch enforces this)
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
  const bool rng = !Mk && keep < 1.f;
  unsigned thr16 = 0; float ik = 1.f;
  if (rng) dropout_spec(keep, &thr16, &ik);
  for (int j0 = 0; j0 < r; j0 += 16) {
    int rch = r - j0;
#define WG(RC, MODE)                                                      \
    lora_wgrad_kernel<RC, MODE><<<grid, DTX_BLOCK, 0, st>>>(              \
        T, (const unsigned short*)X, (const unsigned short*)Mk, part,     \
        M, K, r, j0, splitm, s, seed, thr16, ik)
#define CASE(RC)                                                          \
    do {                                                                  \
      if (Mk) WG(RC, 1);                                                  \
      else if (rng) WG(RC, 2);                                            \
      else WG(RC, 0);                                                     \
    } while (0)
    if (rch <= 4) CASE(4);
    else if (rch <= 8) CASE(8);
    else CASE(16);
#undef CASE
#undef WG
  }
  launch_reduce_partials(part, out, splitm, (long)r * K, st);
}
