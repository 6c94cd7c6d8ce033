// FP8 (OCP e4m3) base GEMMs for LoRA training on CDNA4 (gfx950): the frozen
// weight is quantized once, the activation per call, both with one fp32
// scale per row, and the product runs on the 128-deep fp8 matrix
// instruction at twice the bf16 rate.
//
//   quant_fp8_rows:  x [M,K] bf16 -> q [M,K] e4m3, scale [M] f32
//   gemm_fp8_nt:     C[M,N] bf16 = sa[m] * sb[n] * sum_k A8[m,k] B8[n,k]
//                    (+ src[m,n])
//
// The GEMM is gemm.hip's pipeline restated in bytes (dtx_gemm_pipe.h holds
// the shared pieces): 256x256 tile, 512 threads = 8 waves as 2(M) x 4(N),
// 8 x 4 16x16 fragments per wave, a ring of 5 A + 5 B half-slots of
// [256 rows][64 B] staged by LDS-DMA two tiles ahead with the source-side
// swizzle, counted vmcnt, raw barriers at the ends of p1 and p3, s_setprio
// around the MFMA cluster and both grid orders. A tile's two half-slots now
// hold 2 x 64 fp8 of k, so a tile is K = 128.
//
// One v_mfma_scale_f32_16x16x128_f8f6f4 (unit hardware scales) takes 32
// bytes of k per lane for its row: the lane's 16-byte piece of k-half 0
// (row l & 15, sub-slot l >> 4, the fragment read of gemm.hip) in operand
// registers 0..3 and the same piece of k-half 1 in registers 4..7. Which k
// a (lane, byte) position holds does not matter to a contraction as long as
// A and B agree, and both are read by the same expression.
//
// What differs from the bf16 schedule, and why. Every MFMA reads BOTH
// k-halves, so the phases split the tile by fragment rows, not by k: phase
// p computes fm = 2p, 2p+1 against all four fn (8 MFMAs of 8 passes; B's
// 4 x 32 bytes are read at p0 and kept for the tile). With that
//   - B's two slots of tile kt are dead after p0, so B-kh1 of tile kt+2 may
//     overwrite slot (2kt)%5 at p2 as before;
//   - A's k-half-0 slot of tile kt is still read at p2 and p3, but only its
//     rows of fm 4..7 (rows 64..127 and 192..255). The rows of fm 0..3 are
//     dead after the p1 barrier. So A-kh1 of tile kt+2 is staged in two
//     row sets: the EARLY rows (0..63, 128..191) at kt.p3, the LATE rows
//     one phase later at (kt+1).p0, behind the kt.p3 barrier.
// A wave issues 8 loads per tile as in gemm.hip: at tile kt the late rows
// of tile kt+1 first, then 7 loads of tile kt+2. Loads retire in order, so
// ONE vmcnt(7) at the end of p3 retires all of tile kt+1; the last two
// tiles stage at most the late rows and drain with vmcnt(0).
//
// The scales are applied in fp32 in the epilogue, before the src add and
// the single rounding to bf16.
#include "dtx_gemm_pipe.h"
#include "dtx_launch.h"

typedef __attribute__((ext_vector_type(8))) int int8v;
typedef __attribute__((ext_vector_type(4))) int int4v;

#define FP8_MAX 448.f
#define MFMA_F8(a, b, c)                                                   \
  __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0,       \
                                                   0x7f7f7f7f, 0, 0x7f7f7f7f)

// ------------------------------------------------------------ quantize
// One wave per row, four rows per block. Lane l holds columns
// (i * 64 + l) * 8 .. + 7 for i < NCH as raw bf16 pairs (4 registers per
// chunk) between the absmax pass and the convert: K <= NCH * 512.
#define QUANT_FP8_MAX_K (32 * 512)

template <int NCH>
__global__ __launch_bounds__(256)
void quant_fp8_rows_kernel(const unsigned short* __restrict__ x,
                           unsigned char* __restrict__ q,
                           float* __restrict__ scale, long M, int K) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const unsigned short* xr = x + row * K;
  short8v v[NCH];
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int col = (i * 64 + lane) * 8;
    v[i] = short8v{0, 0, 0, 0, 0, 0, 0, 0};
    if (col < K) v[i] = *reinterpret_cast<const short8v*>(xr + col);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      amax = fmaxf(amax, fabsf(bf2f((unsigned short)v[i][j])));
  }
  amax = wave_reduce_max(amax);
  const float s = amax > 0.f ? amax / FP8_MAX : 1.f;
  if (lane == 0) scale[row] = s;
  unsigned char* qr = q + row * K;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int col = (i * 64 + lane) * 8;
    if (col >= K) continue;
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      f[j] = fminf(fmaxf(bf2f((unsigned short)v[i][j]) / s, -FP8_MAX),
                   FP8_MAX);
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
    uint2v o; o.x = (unsigned)lo; o.y = (unsigned)hi;
    *reinterpret_cast<uint2v*>(qr + col) = o;
  }
}

long quant_fp8_max_k() { return QUANT_FP8_MAX_K; }

void launch_quant_fp8_rows(const void* x, void* q, float* scale, long M,
                           int K, hipStream_t st) {
  dim3 grid((unsigned)DTX_CDIV(M, 4)), block(256);
#define LAUNCH(NCH)                                                        \
  hipLaunchKernelGGL((quant_fp8_rows_kernel<NCH>), grid, block, 0, st,     \
                     (const unsigned short*)x, (unsigned char*)q, scale, M, K)
  if (K <= 2 * 512) LAUNCH(2);
  else if (K <= 8 * 512) LAUNCH(8);
  else LAUNCH(32);
#undef LAUNCH
}

// ---------------------------------------------------------------- GEMM
bool gemm_fp8_supported(long N, long K) {
  return N > 0 && N % 256 == 0 && K % 128 == 0 && K >= 256 &&
         K <= (1L << 23);
}

template <bool HAS_SRC, int GRID>
__global__ __launch_bounds__(512, 2)
void gemm_fp8_nt_kernel(const unsigned char* __restrict__ A,
                        const unsigned char* __restrict__ B,
                        const float* __restrict__ SA,
                        const float* __restrict__ SB,
                        const unsigned short* __restrict__ SRC,
                        unsigned short* __restrict__ C,
                        long M, int N, int K, int mb_n) {
  constexpr int RING = 5;
  constexpr unsigned B_RING = RING * HALF_BYTES;
  __shared__ __attribute__((aligned(16))) unsigned char
      lds[2 * RING * HALF_BYTES];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 2, wn = wid & 3;

  int mb, nb;
  dtx_gemm_block<GRID>(N >> 8, mb_n, mb, nb);
  const long m0 = (long)mb * GEMM_BM;
  const int n0 = nb * GEMM_BN;

  // SRDs rebased per block; num_records clamps the M-tail (loads read 0).
  // Every voffset is below 257 * K, so a record count capped at 2^32 - 1
  // clamps nothing that is addressed.
  const long ldab = K;                                 // A/B row bytes
  const unsigned long long a_bytes = (unsigned long long)(M - m0) * ldab;
  const unsigned long long b_bytes = (unsigned long long)(N - n0) * ldab;
  const uint4v srdA = dtx_srd(
      A + m0 * ldab, a_bytes > 0xffffffffull ? 0xffffffffull : a_bytes);
  const uint4v srdB = dtx_srd(
      B + (long)n0 * ldab, b_bytes > 0xffffffffull ? 0xffffffffull : b_bytes);

  // stage: lane l covers (row = base + l>>2, sub-slot position l&3) of a
  // 16-row piece; the data sub-slot is position ^ f(row bits 2..3).
  const unsigned st_row = lane >> 2;
  const unsigned st_s = (lane & 3) ^ swz_f((lane >> 4) & 3);
  // fragment read: lane l reads row l&15, sub-slot l>>4
  const unsigned fr_off = (lane & 15) * 64
      + ((unsigned)(lane >> 4) ^ swz_f(((lane & 15) >> 2) & 3)) * 16;

  // Whole-half stages: wave wid covers rows wid*32 .. +31 (2 loads).
  const long w_row0 = wid * 32 + st_row;
  const unsigned st_lds = wid * 2048;
  // Row-set stages of A-kh1: wave wid covers ONE 16-row piece, rows
  // (wid>>2)*128 + (wid&3)*16 (+ 64 for the late set).
  const long e_row0 = (wid >> 2) * 128 + (wid & 3) * 16 + st_row;
  const unsigned e_lds = ((wid >> 2) * 128 + (wid & 3) * 16) * 64;

  const int KT = K / 128;

  float4v acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = float4v{0.f, 0.f, 0.f, 0.f};

#define KB(kt, kh) ((long)(kt) * 128 + (kh) * 64 + st_s * 16)
#define STAGE_A(slot, kt, kh)                                               \
  {                                                                         \
    glds16(srdA, (unsigned)(w_row0 * ldab + KB(kt, kh)), (slot) + st_lds);  \
    glds16(srdA, (unsigned)((w_row0 + 16) * ldab + KB(kt, kh)),             \
           (slot) + st_lds + 1024);                                         \
  }
#define STAGE_B(slot, kt, kh)                                               \
  {                                                                         \
    glds16(srdB, (unsigned)(w_row0 * ldab + KB(kt, kh)),                    \
           B_RING + (slot) + st_lds);                                       \
    glds16(srdB, (unsigned)((w_row0 + 16) * ldab + KB(kt, kh)),             \
           B_RING + (slot) + st_lds + 1024);                                \
  }
  // one row set of A-kh1: late = 0 early rows, 1 late rows (+64)
#define STAGE_A1(slot, kt, late)                                            \
  glds16(srdA, (unsigned)((e_row0 + (late) * 64) * ldab + KB(kt, 1)),       \
         (slot) + e_lds + (late) * 4096)
#define SLOT5(h) ((unsigned)((h) % 5) * HALF_BYTES)

  // ---- prologue: tiles 0 and 1 whole (8 loads each, tile 0 first)
  STAGE_B(SLOT5(0), 0, 0); STAGE_A(SLOT5(0), 0, 0);
  STAGE_B(SLOT5(1), 0, 1); STAGE_A(SLOT5(1), 0, 1);
  STAGE_B(SLOT5(2), 1, 0); STAGE_A(SLOT5(2), 1, 0);
  STAGE_B(SLOT5(3), 1, 1); STAGE_A(SLOT5(3), 1, 1);
  dtx_vmcnt8();
  dtx_bar();

  int8v bfr[4];
  int h5 = 0;                          // (2*kt) % 5

  for (int kt = 0; kt < KT; ++kt) {
    const unsigned as0 = (unsigned)h5 * HALF_BYTES;
    const int h5b = h5 + 1 - (h5 + 1 >= 5 ? 5 : 0);
    const unsigned as1 = (unsigned)h5b * HALF_BYTES;   // also (2kt+6) % 5
    const int h5s0 = h5 + 4 - (h5 + 4 >= 5 ? 5 : 0);   // (2kt+4) % 5
    const unsigned ss0 = (unsigned)h5s0 * HALF_BYTES;
    const unsigned ss1 = as0;                          // (2kt+5) % 5
    // slot of tile kt+1's k-half 1: (2kt+3) % 5
    const int h5l = h5 + 3 - (h5 + 3 >= 5 ? 5 : 0);
    const unsigned sl1 = (unsigned)h5l * HALF_BYTES;
    const int kt_s = kt + 2;
    const bool pre = kt_s < KT;
    // tile kt+1's late rows: staged here unless the prologue staged them
    const bool late = kt >= 1 && kt + 1 < KT;
    h5 = h5 + 2 - (h5 + 2 >= 5 ? 5 : 0);

#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (p == 0) {
#pragma unroll
        for (int fn = 0; fn < 4; ++fn) {
          const unsigned o = B_RING + wn * 4096 + fn * 1024 + fr_off;
          const int4v lo = *reinterpret_cast<const int4v*>(&lds[as0 + o]);
          const int4v hi = *reinterpret_cast<const int4v*>(&lds[as1 + o]);
          bfr[fn] = int8v{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        }
      }
      int8v afr[2];
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        const unsigned o = wm * 8192 + (p * 2 + f) * 1024 + fr_off;
        const int4v lo = *reinterpret_cast<const int4v*>(&lds[as0 + o]);
        const int4v hi = *reinterpret_cast<const int4v*>(&lds[as1 + o]);
        afr[f] = int8v{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      }
      // stages of this phase. WAR: ss0 held tile kt-1's k-half 1 (dead
      // since the (kt-1).p3 barrier); ss1 = as0 is THIS tile's k-half 0:
      // its B is dead after p0 (p1 barrier passed at p2), its A rows of
      // fm 0..3 after p1; its A rows of fm 4..7 only after the p3
      // barrier, hence the late set at the next tile's p0.
      if (p == 0) {
        if (late) STAGE_A1(sl1, kt + 1, 1);
        if (pre) STAGE_B(ss0, kt_s, 0)
      } else if (pre) {
        if (p == 1) STAGE_A(ss0, kt_s, 0)
        else if (p == 2) STAGE_B(ss1, kt_s, 1)
        else STAGE_A1(ss1, kt_s, 0);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int fn = 0; fn < 4; ++fn)
          acc[p * 2 + f][fn] = MFMA_F8(afr[f], bfr[fn], acc[p * 2 + f][fn]);
      __builtin_amdgcn_s_setprio(0);
      if (p & 1) {
        if (p == 3) { if (pre) dtx_vmcnt7(); else dtx_vmcnt0(); }
        dtx_bar();
      }
    }
  }
  dtx_vmcnt0();
  dtx_bar();

  // ---- epilogue: f32 through LDS ([256][128] per round, 2 rounds), read
  // coalesced, scale in fp32, (src add), one rounding, buffer stores (rows
  // past M drop on num_records; their sa reads 0).
  const long ldc = (long)N * 2;
  const unsigned long long c_bytes = (unsigned long long)(M - m0) * ldc;
  const int c_rec = (int)(c_bytes > 0xffffffffull ? 0xffffffffu : c_bytes);
  const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(C + m0 * N), (short)0, c_rec, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsS = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(HAS_SRC ? SRC + m0 * N : C), (short)0, HAS_SRC ? c_rec : 0,
      0x00020000);
  const unsigned long long sa_bytes = (unsigned long long)(M - m0) * 4;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(SA + m0), (short)0,
      (int)(sa_bytes > 0xffffffffull ? 0xffffffffu : sa_bytes), 0x00020000);
  float* fl = reinterpret_cast<float*>(lds);

#pragma unroll
  for (int rnd = 0; rnd < 2; ++rnd) {
    if ((wn >> 1) == rnd) {
      const int colb = (wn & 1) * 64 + (lane & 15);
#pragma unroll
      for (int fm = 0; fm < 8; ++fm)
#pragma unroll
        for (int fn = 0; fn < 4; ++fn) {
          const int row = wm * 128 + fm * 16 + (lane >> 4) * 4;
          const int col = colb + fn * 16;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            fl[(row + j) * 128 + col] = acc[fm][fn][j];
        }
    }
    dtx_bar();
    const int col = (tid & 31) * 4;
    const float4v sb = *reinterpret_cast<const float4v*>(
        SB + n0 + rnd * 128 + col);
#pragma unroll
    for (int pass = 0; pass < 16; ++pass) {
      const int row = pass * 16 + (tid >> 5);
      float4v v = *reinterpret_cast<const float4v*>(&fl[row * 128 + col]);
      const float sa = __builtin_bit_cast(
          float, __builtin_amdgcn_raw_buffer_load_b32(rsA, row * 4, 0, 0));
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = v[j] * sa * sb[j];
      const unsigned voff =
          (unsigned)(row * ldc + (n0 + rnd * 128 + col) * 2);
      if (HAS_SRC) {
        uint2v sv = __builtin_amdgcn_raw_buffer_load_b64(rsS, voff, 0, 0);
        v[0] += bf2f((unsigned short)(sv.x & 0xffff));
        v[1] += bf2f((unsigned short)(sv.x >> 16));
        v[2] += bf2f((unsigned short)(sv.y & 0xffff));
        v[3] += bf2f((unsigned short)(sv.y >> 16));
      }
      uint2v out;
      out.x = dtx_cvt_pk_bf16(v[0], v[1]);
      out.y = dtx_cvt_pk_bf16(v[2], v[3]);
      __builtin_amdgcn_raw_buffer_store_b64(out, rsC, voff, 0, 0);
    }
    dtx_bar();
  }
#undef KB
#undef STAGE_A
#undef STAGE_B
#undef STAGE_A1
#undef SLOT5
}

void launch_gemm_fp8_nt(const void* A, const float* SA, const void* B,
                        const float* SB, const void* SRC, void* C, long M,
                        int N, int K, hipStream_t stream) {
  const int mb_n = (int)((M + GEMM_BM - 1) / GEMM_BM);
  const int nb_n = N / GEMM_BN;
  dim3 grid(mb_n * nb_n), block(512);
  // the cluster grid where the block counts divide, else the snake grid
  const bool cluster = (mb_n % 8 == 0) && (nb_n % 4 == 0) && (M % 256 == 0);
#define LAUNCH(HS, G)                                                      \
  hipLaunchKernelGGL((gemm_fp8_nt_kernel<HS, G>), grid, block, 0, stream,  \
                     (const unsigned char*)A, (const unsigned char*)B, SA, \
                     SB, (const unsigned short*)SRC, (unsigned short*)C,   \
                     M, N, K, mb_n)
  if (SRC) { if (cluster) LAUNCH(true, 1); else LAUNCH(true, 2); }
  else     { if (cluster) LAUNCH(false, 1); else LAUNCH(false, 2); }
#undef LAUNCH
}
