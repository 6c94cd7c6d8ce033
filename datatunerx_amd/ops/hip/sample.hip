// Per-row token sampling for serving decode (gfx950): greedy /
// temperature / top-k / top-p with each row's own parameters and its own
// counter-based RNG stream. One 1024-thread workgroup per row.
//
// bf16 logits have at most 65536 distinct values, so nothing is sorted.
// The row sits in registers as packed bf16 (one 16-byte chunk = 8 logits
// = 4 VGPRs, NC <= 19 chunks a thread) and the two cuts are found by
// bisection on the order-preserving 16-bit key of a logit:
//   top-k : the largest key K with  #{key >= K} >= k          (integers)
//   top-p : the largest key K with  mass{key >= K} > p * Z_C  (fp32)
// Each bisection round is one pass over the registers (the weight
// exp2((l - max) * log2e / T) is recomputed, not stored) and one block
// reduction in a FIXED order: per-thread serial, xor-butterfly over the
// wave, a fixed tree over the 16 wave results. No floating-point atomic
// takes part, so a row's token depends on that row's inputs only and is
// bit-reproducible. The tie group of the cut key is admitted by index:
// n = floor((p * Z_C - mass_above) / w_tie) members, located with an
// index-ordered integer scan; the draw is an index-ordered scan of the
// nucleus mass (inverse CDF).
//
// Index order: wave w owns the contiguous chunks [w*cpw, (w+1)*cpw); in
// it chunk (c, lane) = w*cpw + c*64 + lane, so (wave, c, lane, j) is the
// index order and every 16-byte load of a wave is one contiguous KiB.
// Padding chunks hold bf16 NaN (0xFFFF): every comparison with a NaN is
// false, so padding (and a NaN logit) is never a maximum, a candidate or
// a member.
#include "dtx_common.h"
#include "dtx_launch.h"

#define SAMPLE_THREADS 1024
#define SAMPLE_WAVES (SAMPLE_THREADS / WAVE)
#define SAMPLE_INT_MAX 0x7fffffff
// keys of -inf / +inf: the bisection range (every key between them is a
// finite float, so key -> float never makes a NaN threshold)
#define SAMPLE_KEY_NINF 0x007F
#define SAMPLE_KEY_PINF 0xFF80

namespace {

__device__ __forceinline__ float sample_bits_f(unsigned b) {
  union { float f; unsigned i; } x;
  x.i = b;
  return x.f;
}

// order-preserving key of a bf16 value (-0 counts as +0) and its inverse
__device__ __forceinline__ int sample_key_of(float f) {
  union { float f; unsigned i; } x;
  x.f = f;
  unsigned b = x.i >> 16;
  if (b == 0x8000u) b = 0;
  return (int)((b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u));
}

__device__ __forceinline__ float sample_key_f(int key) {
  unsigned k = (unsigned)key;
  unsigned b = (k & 0x8000u) ? (k & 0x7FFFu) : (~k & 0xFFFFu);
  return sample_bits_f(b << 16);
}

// Block- and wave-uniform values come out of LDS or a shuffle, where the
// compiler cannot see that they are uniform: pin them to SGPRs, so the
// bisection loops are scalar loops and the VGPRs stay with the row.
__device__ __forceinline__ int sample_uni(int x) {
  return __builtin_amdgcn_readfirstlane(x);
}

__device__ __forceinline__ float sample_uni(float x) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}

template <typename T>
__device__ __forceinline__ T sample_wave_incl_scan(T x, int lane) {
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    T y = __shfl_up(x, off, WAVE);
    if (lane >= off) x += y;
  }
  return x;
}

__device__ __forceinline__ int sample_wave_sum_i(int x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
  return x;
}

__device__ __forceinline__ int sample_wave_min_i(int x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    x = min(x, __shfl_xor(x, off, WAVE));
  return x;
}

__device__ __forceinline__ int sample_wave_max_i(int x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    x = max(x, __shfl_xor(x, off, WAVE));
  return x;
}

// one fixed tree over the 16 per-wave values
__device__ __forceinline__ float sample_tree16(const float* v) {
  return (((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))) +
         (((v[8] + v[9]) + (v[10] + v[11])) +
          ((v[12] + v[13]) + (v[14] + v[15])));
}

struct SampleShared {
  float f[2][SAMPLE_WAVES];
  int a[2][SAMPLE_WAVES];
  int b[2][SAMPLE_WAVES];
  int bcast;
};

// f(c, j, value, index) over the thread's logits in index order. The
// unpacking shift and mask and the index base go through an empty asm
// once per pass, which makes them opaque: otherwise the compiler hoists
// every element's unpacked value and weight out of the bisection loops
// (they are loop-invariant) and keeps 19 chunk indices live from the
// loads to the last pass, and spills hundreds of VGPRs. The row's own
// registers are never redefined.
template <int NC, class F>
__device__ __forceinline__ void sample_each(const uint4 (&r)[NC], int chunk0,
                                            F f) {
  int sh16 = 16;
  unsigned himask = 0xFFFF0000u;
  asm volatile("" : "+s"(sh16), "+s"(himask), "+v"(chunk0));
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    // every chunk, also the padding of a row shorter than the template
    // holds (NaN: it takes part in nothing)
    const unsigned d[4] = {r[c].x, r[c].y, r[c].z, r[c].w};
    const int base = (chunk0 + c * WAVE) * 8;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f(c, 2 * q, sample_bits_f(d[q] << sh16), base + 2 * q);
      f(c, 2 * q + 1, sample_bits_f(d[q] & himask), base + 2 * q + 1);
    }
    // one chunk at a time: interleaving the chunks' work costs more
    // registers than the row itself
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <int NC>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_kernel(
    const unsigned short* __restrict__ logits, long row_stride, int V,
    const float* __restrict__ temperature, const float* __restrict__ top_p,
    const int* __restrict__ top_k, const long long* __restrict__ seed,
    const int* __restrict__ offset, const float* __restrict__ u_in,
    long long* __restrict__ out) {
  __shared__ SampleShared sh;
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  const unsigned short* x = logits + (long)row * row_stride;

  const int nchunks = V >> 3;
  const int cpw =
      DTX_CDIV(DTX_CDIV(nchunks, SAMPLE_WAVES), WAVE) * WAVE;  // per wave
  const int nrows = cpw / WAVE;                                // <= NC
  const int chunk0 = wid * cpw + lane;  // chunk (c, lane) = chunk0 + c * 64

  uint4 r[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    // clamped, not predicated: the loads of a thread issue back to back
    const int ch = chunk0 + c * WAVE;
    // (uniform row base + 32-bit offset: one address VGPR a load)
    const unsigned off = (unsigned)min(ch, nchunks - 1) * 16u;
    const uint4 v = *reinterpret_cast<const uint4*>(
        reinterpret_cast<const char*>(x) + off);
    r[c] = (c < nrows && ch < nchunks)
               ? v
               : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu,
                            0xFFFFFFFFu);
  }

  int parity = 0;

  // ---- row maximum and its first index (the greedy token) ----
  float lmax = -INFINITY;
  sample_each<NC>(r, chunk0, [&](int, int, float v, int) {
    if (v > lmax) lmax = v;
  });
  lmax = wave_reduce_max(lmax);
  if (lane == 0) sh.f[parity][wid] = lmax;
  __syncthreads();
  {
    float m = sh.f[parity][0];
#pragma unroll
    for (int w = 1; w < SAMPLE_WAVES; ++w) m = fmaxf(m, sh.f[parity][w]);
    lmax = sample_uni(m);
  }
  parity ^= 1;
  int amax = SAMPLE_INT_MAX;
  sample_each<NC>(r, chunk0, [&](int, int, float v, int idx) {
    if (v == lmax) amax = min(amax, idx);
  });
  amax = sample_wave_min_i(amax);
  if (lane == 0) sh.a[parity][wid] = amax;
  __syncthreads();
  {
    int m = sh.a[parity][0];
#pragma unroll
    for (int w = 1; w < SAMPLE_WAVES; ++w) m = min(m, sh.a[parity][w]);
    amax = sample_uni((m < V) ? m : 0);  // an all-NaN row: stay in range
  }
  parity ^= 1;

  const float T = temperature[row];
  if (!(T > 0.f)) {
    if (tid == 0) out[row] = amax;
    return;
  }
  const float scale = 1.4426950408889634f / T;  // weights as exp2
  auto weight = [&](float v) {
    return __builtin_amdgcn_exp2f((v - lmax) * scale);
  };

  // mass{v > t}, #{v > t}, #{v == t}: one pass, one fixed-order reduction
  auto eval = [&](float t, bool with_mass, float& mass_gt, int& cnt_gt,
                  int& cnt_eq) {
    float m = 0.f;
    int g = 0, e = 0;
    if (with_mass) {
      sample_each<NC>(r, chunk0, [&](int, int, float v, int) {
        const bool gt = v > t;
        m += gt ? weight(v) : 0.f;
        g += gt ? 1 : 0;
        e += (v == t) ? 1 : 0;
      });
    } else {
      sample_each<NC>(r, chunk0, [&](int, int, float v, int) {
        g += (v > t) ? 1 : 0;
        e += (v == t) ? 1 : 0;
      });
    }
    m = wave_reduce_sum(m);
    g = sample_wave_sum_i(g);
    e = sample_wave_sum_i(e);
    if (lane == 0) {
      sh.f[parity][wid] = m;
      sh.a[parity][wid] = g;
      sh.b[parity][wid] = e;
    }
    __syncthreads();
    mass_gt = sample_uni(sample_tree16(sh.f[parity]));
    g = 0;
    e = 0;
#pragma unroll
    for (int w = 0; w < SAMPLE_WAVES; ++w) {
      g += sh.a[parity][w];
      e += sh.b[parity][w];
    }
    cnt_gt = sample_uni(g);
    cnt_eq = sample_uni(e);
    parity ^= 1;  // the next call writes the other buffer: one barrier each
  };

  const float p = top_p[row];
  const int k = top_k[row];
  const bool use_k = k > 0 && k < V;
  const bool use_p = p < 1.f;
  const int kmax = min(max(sample_key_of(lmax), SAMPLE_KEY_NINF),
                       SAMPLE_KEY_PINF);

  // The cut: members are v > tcut, plus the first `n_adm` (by index) of
  // the ties v == tcut. Without top-k the candidate cut is the -inf key
  // with its whole (weightless) group.
  int K = SAMPLE_KEY_NINF;
  float mass_gt = 0.f;
  int cnt_gt = 0, cnt_eq = 0, n_adm = 0;
  bool all_ties = true;

  if (use_k) {
    int lo = SAMPLE_KEY_NINF, hi = kmax + 1;  // #{>= lo} >= k > #{>= hi}
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      float mm;
      int g, e;
      eval(sample_key_f(mid), false, mm, g, e);
      if (g + e >= k) lo = mid; else hi = mid;
    }
    K = lo;
  }
  if (use_k || use_p) {
    eval(sample_key_f(K), use_p, mass_gt, cnt_gt, cnt_eq);
    n_adm = use_k ? min(max(k - cnt_gt, 0), cnt_eq) : cnt_eq;
    all_ties = n_adm >= cnt_eq;
  }
  if (use_p) {
    const int n_k = n_adm;
    const int K_k = K;
    const float z_c = mass_gt + (float)n_k * weight(sample_key_f(K_k));
    const float tgt = p * z_c;
    // the rounds need mass{v >= t} only (above K_k every such logit is a
    // candidate): one compare, one exp2, one add a logit; the counts
    // and the split at the cut key come from one eval at the end
    auto mass_ge = [&](float t) {
      float m = 0.f;
      sample_each<NC>(r, chunk0, [&](int, int, float v, int) {
        m += (v >= t) ? weight(v) : 0.f;
      });
      m = wave_reduce_sum(m);
      if (lane == 0) sh.f[parity][wid] = m;
      __syncthreads();
      m = sample_uni(sample_tree16(sh.f[parity]));
      parity ^= 1;
      return m;
    };
    int lo = K_k, hi = kmax + 1;  // mass{>= lo} > tgt >= mass{>= hi}
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (mass_ge(sample_key_f(mid)) > tgt) lo = mid; else hi = mid;
    }
    K = lo;
    if (K != K_k) eval(sample_key_f(K), true, mass_gt, cnt_gt, cnt_eq);
    const int group = (K == K_k) ? n_k : cnt_eq;
    const float w_tie = weight(sample_key_f(K));
    int n = group;
    if (w_tie > 0.f) {
      const float q = floorf((tgt - mass_gt) / w_tie);
      n = (q >= (float)group) ? group : (q > 0.f ? (int)q : 0);
    }
    if (cnt_gt == 0 && n == 0) n = 1;  // never fewer than one token
    n_adm = n;
    all_ties = n_adm >= cnt_eq;
  }
  const float tcut = (use_k || use_p) ? sample_key_f(K) : -INFINITY;

  // ---- index of the last admitted tie (index-ordered integer scan) ----
  int istar = SAMPLE_INT_MAX;
  if (!all_ties) {
    istar = -1;
    if (n_adm > 0) {
      int tot = 0;
      sample_each<NC>(r, chunk0, [&](int, int, float v, int) {
        tot += (v == tcut) ? 1 : 0;
      });
      tot = sample_wave_sum_i(tot);
      if (lane == 0) sh.a[parity][wid] = tot;
      __syncthreads();
      int carry = 0;
#pragma unroll
      for (int w = 0; w < SAMPLE_WAVES; ++w)
        carry += (w < wid) ? sh.a[parity][w] : 0;
      carry = sample_uni(carry);
      parity ^= 1;
      // ties before this chunk < n_adm <= ties through it: exactly one
      // chunk of the row owns the n_adm-th tie
      int cnt = 0;
      sample_each<NC>(r, chunk0, [&](int c, int j, float v, int idx) {
        cnt += (v == tcut) ? 1 : 0;
        if (j == 7) {
          const int incl = sample_wave_incl_scan(cnt, lane) + carry;
          const int excl = incl - cnt;
          if (excl < n_adm && n_adm <= incl) {
            // owner: walk the chunk again for the tie of rank n_adm - 1
            int seen = excl, found = -1;
            const unsigned d[4] = {r[c].x, r[c].y, r[c].z, r[c].w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float ve = (e & 1)
                  ? sample_bits_f(d[e >> 1] & 0xFFFF0000u)
                  : sample_bits_f(d[e >> 1] << 16);
              if (ve == tcut) {
                if (seen == n_adm - 1 && found < 0) found = e;
                ++seen;
              }
            }
            sh.bcast = idx - 7 + found;
          }
          carry = __builtin_amdgcn_readlane(incl, WAVE - 1);
          cnt = 0;
        }
      });
      __syncthreads();
      istar = sample_uni(sh.bcast);
    }
  }
  auto member = [&](float v, int idx) {
    return v > tcut || (v == tcut && idx <= istar);
  };

  // ---- nucleus mass in index order; the last member as the fallback ----
  float tsum = 0.f;
  int last = -1;
  sample_each<NC>(r, chunk0, [&](int, int, float v, int idx) {
    if (member(v, idx)) {
      tsum += weight(v);
      last = idx;
    }
  });
  tsum = wave_reduce_sum(tsum);
  last = sample_wave_max_i(last);
  if (lane == 0) {
    sh.f[parity][wid] = tsum;
    sh.a[parity][wid] = last;
  }
  __syncthreads();
  float woff = 0.f, z_n = 0.f;
#pragma unroll
  for (int w = 0; w < SAMPLE_WAVES; ++w) {
    const float t = sh.f[parity][w];
    if (w < wid) woff += t;
    z_n += t;
    last = max(last, sh.a[parity][w]);
  }
  woff = sample_uni(woff);
  z_n = sample_uni(z_n);
  last = sample_uni(last);
  parity ^= 1;

  float u;
  if (u_in != nullptr) {
    u = u_in[row];
  } else {
    unsigned long long z =
        (unsigned long long)seed[row] +
        ((unsigned long long)(long long)offset[row] + 1ull) * DTX_RNG_GAMMA;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    u = (float)(unsigned)(z >> 40) * 5.9604644775390625e-08f;  // 2^-24
  }
  const float target = sample_uni(u * z_n);

  // ---- inverse CDF: the first chunk (in index order) whose running
  // sum passes target; its owner walks the 8 logits ----
  float carry = woff, csum = 0.f;
  int nmem = 0;
  bool wave_done = false;
  int my_chunk = SAMPLE_INT_MAX, my_tok = -1;
  sample_each<NC>(r, chunk0, [&](int c, int j, float v, int idx) {
    if (member(v, idx)) {
      csum += weight(v);
      ++nmem;
    }
    if (j == 7) {
      const float incl = sample_wave_incl_scan(csum, lane) + carry;
      const bool hit = !wave_done && nmem > 0 && incl > target;
      const unsigned long long ball = __ballot(hit);
      if (ball != 0ull) {
        if (lane == __ffsll((long long)ball) - 1) {
          // the first hit of this wave: walk the chunk from its start
          float run = incl - csum;
          int pick = -1, lastm = -1;
          const unsigned d[4] = {r[c].x, r[c].y, r[c].z, r[c].w};
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float ve = (e & 1)
                ? sample_bits_f(d[e >> 1] & 0xFFFF0000u)
                : sample_bits_f(d[e >> 1] << 16);
            const int ie = idx - 7 + e;
            if (member(ve, ie)) {
              run += weight(ve);
              lastm = ie;
              if (run > target && pick < 0) pick = ie;
            }
          }
          my_chunk = idx >> 3;
          my_tok = pick >= 0 ? pick : lastm;
        }
        wave_done = true;
      }
      carry = __int_as_float(
          __builtin_amdgcn_readlane(__float_as_int(incl), WAVE - 1));
      csum = 0.f;
      nmem = 0;
    }
  });
  const int wave_chunk = sample_wave_min_i(my_chunk);
  if (lane == 0) sh.b[parity][wid] = wave_chunk;
  __syncthreads();
  int first = SAMPLE_INT_MAX;
#pragma unroll
  for (int w = 0; w < SAMPLE_WAVES; ++w) first = min(first, sh.b[parity][w]);
  first = sample_uni(first);
  if (first == SAMPLE_INT_MAX) {
    // rounding left no crossing: the last member (amax when none)
    if (tid == 0) out[row] = (last >= 0 && last < V) ? last : amax;
  } else if (my_chunk == first) {
    out[row] = (my_tok >= 0 && my_tok < V) ? my_tok : amax;
  }
}

}  // namespace

// the register layout holds 19 chunks of 8 logits per thread (76 VGPRs)
long sample_max_vocab() { return 19L * 8 * SAMPLE_THREADS; }

void launch_sample(const void* logits, long row_stride, int B, int V,
                   const float* temperature, const float* top_p,
                   const int* top_k, const long long* seed,
                   const int* offset, const float* u, long long* out,
                   hipStream_t s) {
#define SAMPLE_GO(NC)                                                     \
  sample_kernel<NC><<<B, SAMPLE_THREADS, 0, s>>>(                         \
      (const unsigned short*)logits, row_stride, V, temperature, top_p,   \
      top_k, seed, offset, u, out)
  // the smallest template that holds the row: a pass costs NC chunks
  const int nrows =
      DTX_CDIV(DTX_CDIV(V / 8, SAMPLE_WAVES), WAVE);  // as in the kernel
  if (nrows <= 1) SAMPLE_GO(1);
  else if (nrows <= 2) SAMPLE_GO(2);
  else if (nrows <= 4) SAMPLE_GO(4);
  else if (nrows <= 8) SAMPLE_GO(8);
  else if (nrows <= 12) SAMPLE_GO(12);
  else if (nrows <= 16) SAMPLE_GO(16);
  else SAMPLE_GO(19);
#undef SAMPLE_GO
}
