// GQA-shared MFMA flash-decoding over the bf16 KV cache (gfx950).
//
// attn_decode_kernel (attn_fwd.hip) gives every QUERY head a block of its
// own, so a cache row is fetched G = Hq / Hkv times a token. Here a block
// owns one kv head and one chunk of the cache and serves the G query heads
// of the group as one MFMA operand: a cache row is read once per kv head.
//
// attn_decode_gqa: grid (NS, B*Hkv), 4 waves. A wave takes 32-row kv tiles
// (rows r0 .. r0+31, r0 = chunk start + 32*wave + 128*i).
// mfma_f32_16x16x32_bf16 twice per tile, the operand mapping of
// attn_decode_q8 (docs/kernels.md, "KV cache int8"):
//     S^T[kv, g] = K[kv, :] . Q^T   A = K (global -> registers), B = Q
//     O^T[d, g] += V^T . P^T        A = V^T (LDS transpose read), B = P
// D layout of the MFMA: column = lane % 16, row = 4 * (lane / 16) + reg, so
// the head g sits on lane % 16 in the scores, in P and in the output
// accumulator: running max, sum and the rescale factor are plain registers
// and P feeds the second product from the registers the first left it in.
//   - K: lane (row r, quad h) loads the contiguous D/4 elements h of its K
//     row (D/32 loads of 16 bytes) and the matching elements of q row r.
//     Each 16-byte piece IS an A fragment: the contraction over d is
//     permuted the same way on both sides, nothing is converted or moved.
//   - Score tile t, A row m is kv row (m/4)*8 + t*4 + m%4 of the wave tile:
//     the lane's 8 score registers over the two tiles are kv rows
//     h*8 .. h*8+7, the k order of the PV product's B operand.
//   - q rows >= G are zeros in registers and never loaded.
//   - scale * log2e multiplies the fp32 scores; P is rounded to bf16 once
//     (v_cvt_pk_bf16_f32), the sum l adds the unrounded fp32 values.
//   - V: lane (r, h) loads elements h of rows r and 16 + r the same way and
//     writes them, as loaded, to the wave's own LDS tile [32][D+8] with
//     16-byte stores; ds_read_b64_tr_b16 hands back V^T fragments. Nothing
//     in the loop crosses waves: a wavefront-scope fence orders the tile's
//     writes and reads, there is no workgroup barrier.
//   - Loads are unconditional: row indices are clamped to the chunk's last
//     live row and rows past it take NEG_INF by select before the exp2, so
//     a dead row's bytes are never fetched and p = 0 only ever multiplies a
//     copy of a live V row.
//   - A tile is 64 VGPRs a lane at D = 128 (16 KB a wave), twice the int8
//     kernel's, so the int8 kernel's two tiles in registers do not carry
//     over: two sets cost 256 VGPRs + 32..52 AGPRs (one wave per SIMD) and
//     either 32 v_mov_b64 a tile or, written out as two halves that swap
//     roles, compiler waits inside the math. One set is kept instead. A
//     tile's first acts consume it whole (V to LDS, K through the score
//     MFMAs), the next tile's 16 loads are issued right there into the same
//     registers, and the softmax and the PV product run under them; the one
//     wait sits at the top of the next iteration. 154 VGPRs + 32 AGPRs, two
//     waves per SIMD (D = 64: 98 + 16, four). A wave's last tile issues
//     nothing.
// The four waves meet in LDS in wave order and write one partial per (head,
// chunk) in attn_decode's [B*Hq, NS, D+2] format; its combine kernel
// finishes o and lse. A chunk at or past the live length writes the neutral
// partial (m = NEG_INF, l = 0, o = 0).
//
// Build: no packed fp32 VALU instructions in this file, switched off in the
// device pass for the whole translation unit as kvq.hip does and for its
// reasons (thread and block ids through the builtins, the grid size as a
// kernel argument). When editing: the listing must hold no v_pk_*_f32 and
// no s_swappc.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                              \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "dtx_mfma.h"
#include "dtx_launch.h"

#define GD_TID ((int)__builtin_amdgcn_workitem_id_x())
#define GD_BIDX ((int)__builtin_amdgcn_workgroup_id_x())
#define GD_BIDY ((int)__builtin_amdgcn_workgroup_id_y())

typedef __attribute__((ext_vector_type(2))) float gd_f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 gd_bf16x2;

// two floats -> packed bf16 pair (RNE, one v_cvt_pk_bf16_f32), lo in
// bits 0..15; plain code, so the scheduler may place it.
__device__ __forceinline__ unsigned gd_pack_bf16(float lo, float hi) {
  const gd_f32x2 f = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f, gd_bf16x2));
}

// Orders a wave's own LDS traffic (the LDS serves a wave in order; this
// keeps the compiler from moving a read across a write of another lane).
__device__ __forceinline__ void gd_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// The loop's wave-private V tiles and the epilogue's cross-wave image share
// the storage: one workgroup barrier separates them.
template <int D>
union GqaLds {
  unsigned short v[4][32][D + 8];      // V tile, per wave
  float red[4][16][D + 4];             // o[D], m, l per (wave, head)
};

template <int D>
__global__ __launch_bounds__(256)
void attn_decode_gqa_kernel(const unsigned short* __restrict__ Q,
                            const unsigned short* __restrict__ Kp,
                            const unsigned short* __restrict__ Vp,
                            const int* __restrict__ len_dev,
                            float* __restrict__ part,   // [B*Hq, NS, D+2]
                            int Hq, int Hkv, int Skv, long bstride,
                            int chunk, int NS, int len_stride,
                            float kscale) {
  constexpr int EPL = D / 4;           // elements of a cache row per lane
  constexpr int NL = EPL / 8;          // 16-byte loads per lane per row
                                       // = MFMA k-steps of the scores
  constexpr int NDT = D / 16;          // 16-row d tiles of O^T
  constexpr int VSTR = D + 8;
  __shared__ GqaLds<D> lds;

  const int lane = GD_TID & 63;
  const int wid = __builtin_amdgcn_readfirstlane(GD_TID >> 6);
  const int r = lane & 15, h = lane >> 4;
  const int G = Hq / Hkv;
  const int b = GD_BIDY / Hkv, hkv = GD_BIDY % Hkv;
  const int len = min(len_dev ? len_dev[b * len_stride] : Skv, Skv);
  const int kv0 = GD_BIDX * chunk;
  // head g of the group: + g * NS * (D + 2)
  float* pblk = part + ((long)(b * Hq + hkv * G) * NS + GD_BIDX) * (D + 2);
  const long phead = (long)NS * (D + 2);

  if (kv0 >= len) {                    // nothing live here: neutral partial
    for (int i = GD_TID; i < G * (D + 2); i += 256) {
      const int c = i % (D + 2);
      pblk[(i / (D + 2)) * phead + c] = c == D ? NEG_INF : 0.f;
    }
    return;
  }
  const int kv_end = min(len, kv0 + chunk);
  const int last = kv_end - 1;

  // q rows of the group as B fragments; rows >= G are zeros, never loaded
  short8v qf[NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    qf[j] = (short8v){0, 0, 0, 0, 0, 0, 0, 0};
    if (r < G)
      qf[j] = *reinterpret_cast<const short8v*>(
          Q + ((long)b * Hq + hkv * G + r) * D + h * EPL + j * 8);
  }

  const long rowstr = (long)Hkv * D;
  const long cbase = (long)b * bstride + (long)hkv * D + h * EPL;
  const unsigned short* kb = Kp + cbase;
  const unsigned short* vb = Vp + cbase;
  const int krow = (r >> 2) * 8 + (r & 3);         // + t * 4

  // one wave tile in flight: the lane's K fragments and V pieces
  struct Tile { short8v k[2][NL], v[2][NL]; };
  auto issue = [&](Tile& x, int r0) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const unsigned short* kp =
          kb + (long)min(r0 + krow + t * 4, last) * rowstr;
      const unsigned short* vp =
          vb + (long)min(r0 + t * 16 + r, last) * rowstr;
#pragma unroll
      for (int n = 0; n < NL; ++n) {
        x.k[t][n] = *reinterpret_cast<const short8v*>(kp + n * 8);
        x.v[t][n] = *reinterpret_cast<const short8v*>(vp + n * 8);
      }
    }
  };
  // a use of every loaded register: the wait for the loads lands here
  auto settle = [&](Tile& x) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int n = 0; n < NL; ++n)
        asm volatile("" : "+v"(x.k[t][n]), "+v"(x.v[t][n]));
  };

  float m_run = NEG_INF, l_run = 0.f;  // l_run: this lane's 8 rows a tile
  f32x4 oacc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) oacc[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  DTX_AS3 unsigned short* vt = (DTX_AS3 unsigned short*)&lds.v[wid][0][0];
  // 16-byte writes: row t*16 + r, the lane's EPL columns
  DTX_AS3 unsigned short* vw = vt + r * VSTR + h * EPL;
  // transpose read: the 16-lane group h gets rows h*8 .. +3 (then +4 .. +7)
  // of 16 columns, lane r column r
  const int troff = (h * 8 + ((lane >> 2) & 3)) * VSTR + (lane & 3) * 4;

  // One register set: the tile is waited for (settle), consumed by the LDS
  // stores and the score MFMAs, and refilled at once; the rest of the
  // iteration runs under the loads and the compiler places no wait of its
  // own in it. wid and kv_end are wave-uniform, so the branches are scalar
  // and every lane reaches every MFMA.
  int r0 = kv0 + wid * 32;
  Tile x;
  issue(x, r0);
  for (; r0 < kv_end; r0 += 128) {
    settle(x);
    gd_wave_sync();                    // the previous tile's reads are done
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int n = 0; n < NL; ++n)
        *reinterpret_cast<DTX_AS3 short8v*>(vw + t * 16 * VSTR + n * 8) =
            x.v[t][n];
    gd_wave_sync();

    // S^T[kv, g], fp32 accumulate
    f32x4 s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      s[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < NL; ++j) s[t] = MFMA16(x.k[t][j], qf[j], s[t]);
    }
    if (r0 + 128 < kv_end) issue(x, r0 + 128);   // x is dead: refill it

    // this lane: kv rows r0 + h*8 + j, head lane % 16
    float sv[8];
    float mx = NEG_INF;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float val = s[j >> 2][j & 3] * kscale;
      sv[j] = r0 + h * 8 + j < kv_end ? val : NEG_INF;
      mx = fmaxf(mx, sv[j]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));      // row r0 is live: finite
    const float m_new = fmaxf(m_run, mx);
    const float alpha = __builtin_exp2f(m_run - m_new);
    float ps = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sv[j] = __builtin_exp2f(sv[j] - m_new);
      ps += sv[j];
    }
    l_run = l_run * alpha + ps;
    m_run = m_new;
    union { unsigned u[4]; short8v v; } pf;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      pf.u[j] = gd_pack_bf16(sv[2 * j], sv[2 * j + 1]);

    // O^T[d, g] = alpha[g] * O^T + V^T . P^T
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      union { bf16x4 q[2]; short8v v; } vf;
      vf.q[0] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
          (DTX_AS3 bf16x4*)(vt + troff + dt * 16));
      vf.q[1] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
          (DTX_AS3 bf16x4*)(vt + troff + dt * 16 + 4 * VSTR));
#pragma unroll
      for (int e = 0; e < 4; ++e) oacc[dt][e] *= alpha;
      oacc[dt] = MFMA16(vf.v, pf.v, oacc[dt]);
    }
  }

  // the lane quads of a head hold disjoint rows: one sum per head
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
  __syncthreads();                     // tiles are dead, red aliases them
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
    *reinterpret_cast<f32x4*>(&lds.red[wid][r][dt * 16 + 4 * h]) = oacc[dt];
  if (h == 0) {
    lds.red[wid][r][D] = m_run;
    lds.red[wid][r][D + 1] = l_run;
  }
  __syncthreads();
  // waves in order 0..3; wave 0 always has a live row, so m_all is finite.
  // m leaves the exp2 domain here: the partial holds natural-log units.
  for (int i = GD_TID; i < G * D; i += 256) {
    const int g = i / D, d = i % D;
    float m_all = lds.red[0][g][D];
#pragma unroll
    for (int w = 1; w < 4; ++w) m_all = fmaxf(m_all, lds.red[w][g][D]);
    float o = 0.f, l = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float wt = __builtin_exp2f(lds.red[w][g][D] - m_all);
      o += wt * lds.red[w][g][d];
      l += wt * lds.red[w][g][D + 1];
    }
    float* pg = pblk + g * phead;
    pg[d] = o;
    if (d == 0) {
      pg[D] = m_all * LN2;
      pg[D + 1] = l;
    }
  }
}

bool gqa_decode_supported(int Hq, int Hkv, int D) {
  return (D == 64 || D == 128) && Hkv >= 1 && Hq >= 1 && Hq % Hkv == 0 &&
         Hq / Hkv >= 2 && Hq / Hkv <= 16;
}

// Chunks are whole wave rounds (4 waves x 32 rows: 64 KiB of cache at
// D = 128, 32 KiB at D = 64), cut so that one batch row alone gives about
// two blocks per CU (256 CUs) where the capacity allows, and at most 32 of
// them: the combine walks a head's partials one after the other, and at 64
// chunks that walk cost more than the finer cut won (profiles/README.md,
// "KV cache int8"). Never a function of B or of the live lengths: a row's
// summation order must not depend on the batch it sits in.
int attn_decode_gqa_chunk(int Skv, int Hkv, int D) {
  (void)D;
  int ns = DTX_CDIV(512, Hkv);
  if (ns > 32) ns = 32;
  const int chunk = DTX_CDIV(DTX_CDIV(Skv, ns), 128) * 128;
  return chunk < 128 ? 128 : chunk;
}

int attn_decode_gqa_nsplit(int Skv, int Hkv, int D) {
  const int ns = DTX_CDIV(Skv, attn_decode_gqa_chunk(Skv, Hkv, D));
  return ns < 1 ? 1 : ns;
}

void launch_attn_decode_gqa(const void* q, const void* k, const void* v,
                            const int* len_dev, float* part, void* o,
                            float* lse, int B, int Hq, int Hkv, int Skv,
                            int D, float scale, int len_stride,
                            hipStream_t st) {
  const int chunk = attn_decode_gqa_chunk(Skv, Hkv, D);
  const int ns = attn_decode_gqa_nsplit(Skv, Hkv, D);
  const long bstride = (long)Skv * Hkv * D;
  dim3 grid(ns, B * Hkv);
#define DTX_GQA_DECODE(DD)                                                 \
  attn_decode_gqa_kernel<DD><<<grid, 256, 0, st>>>(                        \
      (const unsigned short*)q, (const unsigned short*)k,                  \
      (const unsigned short*)v, len_dev, part, Hq, Hkv, Skv, bstride,      \
      chunk, ns, len_stride, scale * LOG2E)
  if (D == 128) DTX_GQA_DECODE(128);
  else if (D == 64) DTX_GQA_DECODE(64);
  else return;
#undef DTX_GQA_DECODE
  launch_attn_decode_combine(part, o, lse, B * Hq, ns, D, st);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
