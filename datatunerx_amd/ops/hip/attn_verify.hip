// Multi-token verify attention over the bf16 KV cache (gfx950): the
// attention of a speculative-decoding step. T new tokens of a sequence are
// already in the cache and each attends the live prefix up to itself.
//
// attn_verify: q [B,T,Hq,D], cache k, v [Bc,cap,Hkv,D], len[b] = live rows
// INCLUDING the T new ones, read on the device and clamped to cap. Query t
// of row b sees kv rows j <= len[b] - T + t (bottom-right-aligned causal).
// len[b] < T is the caller's error and is defined: a query whose limit is
// negative sees nothing and gets o = 0 and lse = NEG_INF + log(1e-30) from
// the combine; no address depends on the queries, so nothing is read
// outside the cache.
//
// The kernel is attn_decode_gqa's with wider B operands. A block owns one
// kv head and one chunk of the cache (grid (NS, B*Hkv), 4 waves, 32-row kv
// tiles per wave, the sibling's split plan), and the MFMA columns are the
// (t, g) pairs of that kv head, column c = t * G + g, C = T * G <= 32:
//     S^T[kv, c] = K[kv, :] . Q^T   A = K (global -> registers), B = Q
//     O^T[d, c] += V^T . P^T        A = V^T (LDS transpose read), B = P
// NCT = 1 or 2 column tiles of 16, a template parameter. The K fragments
// and the V^T fragments of a tile are loaded once and feed the MFMAs of
// both column tiles: a cache row is read once per kv head per step,
// whatever T and G are. Operand mapping, the wave-private V tile in LDS,
// ds_read_b64_tr_b16, clamped unconditional loads and the one register set
// in flight are the sibling's; see its header. What differs:
//   - The causal limit is per column: column c sees rows below
//     vis[c] = max(len - T + t + 1, 0). Only wave tiles that reach past
//     len - T + 1 (the smallest limit) compare against min(vis[c], kv_end);
//     interior tiles take the sibling's row < kv_end select and no more.
//     The choice is wave-uniform.
//   - A column may see no row of a tile, or of the whole chunk, while its
//     neighbours do (the new rows straddle a chunk boundary). Visible rows
//     are a prefix, so such a column has either seen rows before (finite
//     running max: p = exp2(NEG_INF - m) = 0) or none at all: then the max
//     stays NEG_INF and the exponent's reference is 0, never NEG_INF:
//     alpha = p = exp2(NEG_INF - 0) = 0, and l and o stay 0. The block
//     epilogue writes the exact neutral partial (m = NEG_INF, l = 0,
//     o = 0) for a column no wave saw a row for.
//   - Rows in [vis[c], len) are live (the later new tokens): p = 0
//     multiplies real V rows there; rows >= len are never fetched.
//   - Columns >= C are zero q rows, computed and never written.
//   - The epilogue runs once per column tile over the same LDS image.
// Partials go to attn_decode's [rows, NS, D+2] format with row =
// (b * T + t) * Hq + head, so its combine kernel writes o as [B,T,Hq,D]
// and lse as [B,T,Hq].
//
// Registers: the sibling's one tile in flight is 154 VGPRs + 32 AGPRs at
// D = 128; a second column tile adds 16 (q) + 32 (accumulator) + 16
// (scores) and must stay within two waves per SIMD (256 in all), which
// __launch_bounds__(256, 2) asks for. The listing (hipcc
// --offload-arch=gfx950 -O3), VGPRs + AGPRs, waves per SIMD, no spill and
// no scratch in any of them:
//   D = 128: NCT = 1  157 + 0, 3     NCT = 2  217 + 0, 2
//   D =  64: NCT = 1   95 + 0, 5     NCT = 2  137 + 0, 3
//
// Build: no packed fp32 VALU instructions, as attn_decode_gqa.hip and for
// its reasons. When editing: the listing must hold no v_pk_*_f32, no
// s_swappc and no scratch.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                              \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "dtx_mfma.h"
#include "dtx_launch.h"

#define AV_TID ((int)__builtin_amdgcn_workitem_id_x())
#define AV_BIDX ((int)__builtin_amdgcn_workgroup_id_x())
#define AV_BIDY ((int)__builtin_amdgcn_workgroup_id_y())

typedef __attribute__((ext_vector_type(2))) float av_f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 av_bf16x2;

// two floats -> packed bf16 pair (RNE, one v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned av_pack_bf16(float lo, float hi) {
  const av_f32x2 f = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f, av_bf16x2));
}

// Orders a wave's own LDS traffic.
__device__ __forceinline__ void av_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <int D>
union VerifyLds {
  unsigned short v[4][32][D + 8];      // V tile, per wave
  float red[4][16][D + 4];             // o[D], m, l per (wave, column)
};

template <int D, int NCT>
__global__ __launch_bounds__(256, 2)
void attn_verify_kernel(const unsigned short* __restrict__ Q,
                        const unsigned short* __restrict__ Kp,
                        const unsigned short* __restrict__ Vp,
                        const int* __restrict__ len_dev,
                        float* __restrict__ part,   // [B*T*Hq, NS, D+2]
                        int T, int Hq, int Hkv, int Skv, long bstride,
                        int chunk, int NS, int len_stride, float kscale) {
  constexpr int EPL = D / 4;           // elements of a cache row per lane
  constexpr int NL = EPL / 8;          // 16-byte loads per lane per row
  constexpr int NDT = D / 16;          // 16-row d tiles of O^T
  constexpr int VSTR = D + 8;
  __shared__ VerifyLds<D> lds;

  const int lane = AV_TID & 63;
  const int wid = __builtin_amdgcn_readfirstlane(AV_TID >> 6);
  const int r = lane & 15, h = lane >> 4;
  const int G = Hq / Hkv, C = T * G;
  const int b = AV_BIDY / Hkv, hkv = AV_BIDY % Hkv;
  const int len = min(len_dev ? len_dev[b * len_stride] : Skv, Skv);
  const int kv0 = AV_BIDX * chunk;
  // partial of column (t, g): row (b*T + t)*Hq + hkv*G + g, plane AV_BIDX
  const long phead = (long)NS * (D + 2);
  float* pblk = part + ((long)b * T * Hq + hkv * G) * phead +
                (long)AV_BIDX * (D + 2);
  auto pcol = [&](int col) {
    return pblk + ((long)(col / G) * Hq + col % G) * phead;
  };

  if (kv0 >= len) {                    // nothing live here: neutral partials
    for (int i = AV_TID; i < C * (D + 2); i += 256) {
      const int c = i % (D + 2);
      pcol(i / (D + 2))[c] = c == D ? NEG_INF : 0.f;
    }
    return;
  }
  const int kv_end = min(len, kv0 + chunk);
  const int last = kv_end - 1;
  const int vis_min = len - T + 1;     // query 0's limit: the smallest

  // q rows of the lane's columns as B fragments; columns >= C are zeros.
  // vlim: rows of this chunk the column sees are those below it.
  short8v qf[NCT][NL];
  int vlim[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    const int col = ct * 16 + r;
    const int t = min(col / G, T - 1);
    vlim[ct] = min(max(len - T + t + 1, 0), kv_end);
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      qf[ct][j] = (short8v){0, 0, 0, 0, 0, 0, 0, 0};
      if (col < C)
        qf[ct][j] = *reinterpret_cast<const short8v*>(
            Q + (((long)b * T + t) * Hq + hkv * G + col % G) * D + h * EPL +
            j * 8);
    }
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

  float m_run[NCT], l_run[NCT];        // l_run: this lane's 8 rows a tile
  f32x4 oacc[NCT][NDT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    m_run[ct] = NEG_INF;
    l_run[ct] = 0.f;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
      oacc[ct][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  DTX_AS3 unsigned short* vt = (DTX_AS3 unsigned short*)&lds.v[wid][0][0];
  DTX_AS3 unsigned short* vw = vt + r * VSTR + h * EPL;
  const int troff = (h * 8 + ((lane >> 2) & 3)) * VSTR + (lane & 3) * 4;

  int r0 = kv0 + wid * 32;
  Tile x;
  issue(x, r0);
  for (; r0 < kv_end; r0 += 128) {
    settle(x);
    av_wave_sync();                    // the previous tile's reads are done
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int n = 0; n < NL; ++n)
        *reinterpret_cast<DTX_AS3 short8v*>(vw + t * 16 * VSTR + n * 8) =
            x.v[t][n];
    av_wave_sync();

    // S^T[kv, c]: every K fragment serves both column tiles
    f32x4 s[NCT][2];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int t = 0; t < 2; ++t)
        s[ct][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < NL; ++j)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
          s[ct][t] = MFMA16(x.k[t][j], qf[ct][j], s[ct][t]);
    if (r0 + 128 < kv_end) issue(x, r0 + 128);   // x is dead: refill it

    // The causal limit only where the tile reaches the last T live rows.
    const bool tail = r0 + 32 > vis_min;         // wave-uniform
    union { unsigned u[4]; short8v v; } pf[NCT];
    float alpha[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      const int lim = tail ? vlim[ct] : kv_end;
      // this lane: kv rows r0 + h*8 + j, column ct*16 + lane % 16
      float sv[8];
      float mx = NEG_INF;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float val = s[ct][j >> 2][j & 3] * kscale;
        sv[j] = r0 + h * 8 + j < lim ? val : NEG_INF;
        mx = fmaxf(mx, sv[j]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run[ct], mx);
      // a column that has seen no row yet: reference 0, so p = alpha = 0
      const float m_ref = m_new == NEG_INF ? 0.f : m_new;
      alpha[ct] = __builtin_exp2f(m_run[ct] - m_ref);
      float ps = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        sv[j] = __builtin_exp2f(sv[j] - m_ref);
        ps += sv[j];
      }
      l_run[ct] = l_run[ct] * alpha[ct] + ps;
      m_run[ct] = m_new;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        pf[ct].u[j] = av_pack_bf16(sv[2 * j], sv[2 * j + 1]);
    }

    // O^T[d, c] = alpha[c] * O^T + V^T . P^T: every V^T fragment serves
    // both column tiles
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      union { bf16x4 q[2]; short8v v; } vf;
      vf.q[0] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
          (DTX_AS3 bf16x4*)(vt + troff + dt * 16));
      vf.q[1] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
          (DTX_AS3 bf16x4*)(vt + troff + dt * 16 + 4 * VSTR));
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
        for (int e = 0; e < 4; ++e) oacc[ct][dt][e] *= alpha[ct];
        oacc[ct][dt] = MFMA16(vf.v, pf[ct].v, oacc[ct][dt]);
      }
    }
  }

  // The four waves meet in LDS, one column tile at a time. m leaves the
  // exp2 domain here: the partial holds natural-log units.
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    float l = l_run[ct];               // the lane quads hold disjoint rows
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    __syncthreads();                   // V tiles / the last image are dead
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
      *reinterpret_cast<f32x4*>(&lds.red[wid][r][dt * 16 + 4 * h]) =
          oacc[ct][dt];
    if (h == 0) {
      lds.red[wid][r][D] = m_run[ct];
      lds.red[wid][r][D + 1] = l;
    }
    __syncthreads();
    const int ncol = min(16, C - ct * 16);
    for (int i = AV_TID; i < ncol * D; i += 256) {
      const int c = i / D, d = i % D;
      float m_all = lds.red[0][c][D];
#pragma unroll
      for (int w = 1; w < 4; ++w) m_all = fmaxf(m_all, lds.red[w][c][D]);
      const bool empty = m_all == NEG_INF;   // no wave saw a row: neutral
      float o = 0.f, lsum = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float wt =
            empty ? 0.f : __builtin_exp2f(lds.red[w][c][D] - m_all);
        o += wt * lds.red[w][c][d];
        lsum += wt * lds.red[w][c][D + 1];
      }
      float* pg = pcol(ct * 16 + c);
      pg[d] = o;
      if (d == 0) {
        pg[D] = empty ? NEG_INF : m_all * LN2;
        pg[D + 1] = lsum;
      }
    }
  }
}

bool attn_verify_supported(int T, int Hq, int Hkv, int D) {
  return (D == 64 || D == 128) && Hkv >= 1 && Hq >= 1 && Hq % Hkv == 0 &&
         T >= 1 && T <= 16 && (long)T * (Hq / Hkv) <= 32;
}

// The sibling's split plan: the blocks do the same work per cache row, so
// the same cut fills the chip; a function of the addressed capacity and
// the head shape alone.
int attn_verify_chunk(int Skv, int Hkv, int D) {
  return attn_decode_gqa_chunk(Skv, Hkv, D);
}

int attn_verify_nsplit(int Skv, int Hkv, int D) {
  return attn_decode_gqa_nsplit(Skv, Hkv, D);
}

void launch_attn_verify(const void* q, const void* k, const void* v,
                        const int* len_dev, float* part, void* o,
                        float* lse, int B, int T, int Hq, int Hkv, int Skv,
                        int D, float scale, int len_stride,
                        hipStream_t st) {
  const int chunk = attn_verify_chunk(Skv, Hkv, D);
  const int ns = attn_verify_nsplit(Skv, Hkv, D);
  const long bstride = (long)Skv * Hkv * D;
  const bool two = T * (Hq / Hkv) > 16;
  dim3 grid(ns, B * Hkv);
#define DTX_ATTN_VERIFY(DD, NCT)                                           \
  attn_verify_kernel<DD, NCT><<<grid, 256, 0, st>>>(                       \
      (const unsigned short*)q, (const unsigned short*)k,                  \
      (const unsigned short*)v, len_dev, part, T, Hq, Hkv, Skv, bstride,   \
      chunk, ns, len_stride, scale * LOG2E)
  if (D == 128 && two) DTX_ATTN_VERIFY(128, 2);
  else if (D == 128) DTX_ATTN_VERIFY(128, 1);
  else if (D == 64 && two) DTX_ATTN_VERIFY(64, 2);
  else if (D == 64) DTX_ATTN_VERIFY(64, 1);
  else return;
#undef DTX_ATTN_VERIFY
  launch_attn_decode_combine(part, o, lse, B * T * Hq, ns, D, st);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
