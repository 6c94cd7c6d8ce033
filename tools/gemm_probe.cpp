// Standalone A/B probe for the hand-written NT GEMM (no torch): the two
// shipped block grids (g1p2 = 8x4 clusters, g2p2 = snake row-groups) run
// interleaved in ONE process (guide §5.4 rule 24), random data (rule
// 25), bitwise cross-check between them (same math order => identical
// bits).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/gemm_probe.cpp -o tools/gemm_probe.bin
//   ./tools/gemm_probe.bin bench 24576 4096 4096 [rounds]
//   ./tools/gemm_probe.bin one <0=g1p2|1=g2p2> 24576 4096 4096 <iters>   # for rocprofv3
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <chrono>

#include "../datatunerx_amd/ops/hip/gemm.hip"

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { \
  fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e), \
          __FILE__, __LINE__); exit(1); } } while (0)

__global__ void fill_rand(unsigned short* p, long n, unsigned seed) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned long long z = seed + (unsigned long long)i * 0x9E3779B97F4A7C15ull;
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27;
  float f = ((z >> 40) & 0xFFFFFF) / 8388608.0f * 2.f - 1.f;  // [-1,1)
  union { float f; unsigned u; } u; u.f = f;
  p[i] = (unsigned short)(u.u >> 16);
}

template <int GRID>
void run(const unsigned short* A, const unsigned short* B,
         unsigned short* C, long M, int N, int K) {
  const int mb_n = (int)((M + 255) / 256), nb_n = N / 256;
  hipLaunchKernelGGL((gemm_nt_kernel<false, GRID>),
                     dim3(mb_n * nb_n),
                     dim3(512), 0, 0, A, B, nullptr, C, M, N, K, mb_n);
}

typedef void (*runfn)(const unsigned short*, const unsigned short*,
                      unsigned short*, long, int, int);
#define NVAR 2
static runfn FNS[NVAR] = {run<1>, run<2>};
static const char* NAMES[NVAR] = {"g1p2", "g2p2"};

int main(int argc, char** argv) {
  const bool one = argc > 1 && !strcmp(argv[1], "one");
  if (argc < (one ? 6 : 5)) {
    fprintf(stderr, "usage: see header\n");
    return 1;
  }
  int ai = one ? 3 : 2;  // one <grid> M N K [iters]
  long M = atol(argv[ai]); int N = atoi(argv[ai + 1]), K = atoi(argv[ai + 2]);
  int rounds = argc > ai + 3 ? atoi(argv[ai + 3]) : 6;

  const bool cluster_ok = (M / 256) % 8 == 0 && (N / 256) % 4 == 0
                          && M % 256 == 0;
  if (M <= 0 || N <= 0 || N % 256 || K <= 0 || K % 64) {
    fprintf(stderr, "need N %% 256 == 0 and K %% 64 == 0\n");
    return 1;
  }

  unsigned short *A, *B, *C;
  CK(hipMalloc(&A, M * (long)K * 2));
  CK(hipMalloc(&B, (long)N * K * 2));
  CK(hipMalloc(&C, M * (long)N * 2));
  hipLaunchKernelGGL(fill_rand, dim3((M * K + 255) / 256), dim3(256), 0, 0,
                     A, M * (long)K, 1u);
  hipLaunchKernelGGL(fill_rand, dim3(((long)N * K + 255) / 256), dim3(256),
                     0, 0, B, (long)N * K, 2u);
  CK(hipDeviceSynchronize());
  const double fl = 2.0 * M * N * K;

  if (one) {
    int g = atoi(argv[2]);
    if (g < 0 || g >= NVAR || (g == 0 && !cluster_ok)) {
      fprintf(stderr, "grid %d not valid for this shape\n", g);
      return 1;
    }
    for (int i = 0; i < rounds; ++i) FNS[g](A, B, C, M, N, K);
    CK(hipDeviceSynchronize());
    printf("done %s\n", NAMES[g]);
    return 0;
  }

  // bitwise cross-check of the cluster grid against the snake grid
  if (cluster_ok) {
    std::vector<unsigned short> ref(4096), got(4096);
    FNS[1](A, B, C, M, N, K);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(ref.data(), C + M * (long)N / 2, 8192,
                 hipMemcpyDeviceToHost));
    CK(hipMemset(C + M * (long)N / 2, 0, 8192));
    FNS[0](A, B, C, M, N, K);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(got.data(), C + M * (long)N / 2, 8192,
                 hipMemcpyDeviceToHost));
    if (memcmp(ref.data(), got.data(), 8192))
      printf("MISMATCH %s vs %s: not bitwise equal\n", NAMES[0], NAMES[1]);
  }

  double best[NVAR] = {1e30, 1e30};
  for (int r = 0; r < rounds; ++r)
    for (int v = 0; v < NVAR; ++v) {
      if (v == 0 && !cluster_ok) continue;
      CK(hipDeviceSynchronize());
      auto t0 = std::chrono::steady_clock::now();
      for (int i = 0; i < 3; ++i) FNS[v](A, B, C, M, N, K);
      CK(hipDeviceSynchronize());
      double dt = std::chrono::duration<double>(
                      std::chrono::steady_clock::now() - t0).count() / 3;
      if (dt < best[v]) best[v] = dt;
    }
  for (int v = 0; v < NVAR; ++v)
    if (best[v] < 1e29)
      printf("%s  M=%ld N=%d K=%d  %7.3f ms  %7.1f TF/s\n", NAMES[v], M, N,
             K, best[v] * 1e3, fl / best[v] / 1e12);
  return 0;
}
