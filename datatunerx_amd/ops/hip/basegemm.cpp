// Frozen-base GEMM on hipBLASLt with C != D:
//   D[M,N] = A[M,K] @ B[N,K]^T + C[M,N], bf16 in and out, fp32 accumulate.
// torch.addmm(c, a, b.t()) computes the same thing by first copying c into
// the result and then running the GEMM in place with beta = 1; hipBLASLt
// reads C and writes D as two buffers, so the copy (one full pass over the
// residual per o_proj / down_proj call) is not needed.
//
// In the library's column-major terms this is the F.linear call: transA = T
// on B (ld K), transB = N on A (ld K), C and D [N x M] with ld N, so it runs
// the forward-layout kernels. Host-only, no torch (see dtx_launch.h).
#include <hipblaslt/hipblaslt.h>
#include <hipblaslt/hipblaslt-version.h>

#include <map>
#include <mutex>
#include <tuple>

#include "dtx_launch.h"

namespace {

// Everything hipBLASLt needs for one (device, M, N, K): built on the first
// call of the shape, never freed (a training run has a handful of shapes).
struct Plan {
  hipblasLtMatmulDesc_t desc = nullptr;
  hipblasLtMatrixLayout_t la = nullptr, lb = nullptr, lc = nullptr;
  hipblasLtMatmulAlgo_t algo;
};

std::mutex g_mu;
std::map<int, hipblasLtHandle_t> g_handles;              // per device
std::map<int, int> g_versions;            // the loaded library's, per device
std::map<std::tuple<int, int, int, int>, Plan> g_plans;  // device, M, N, K

#define LT_TRY(call)                                  \
  do {                                                \
    const hipblasStatus_t st_ = (call);               \
    if (st_ != HIPBLAS_STATUS_SUCCESS) {              \
      *failed = #call;                                \
      return (int)st_;                                \
    }                                                 \
  } while (0)

// Fills `plan` for the shape; on failure names the call and leaves a plan
// that is not cached.
int make_plan(hipblasLtHandle_t h, int M, int N, int K, size_t ws_bytes,
              Plan* plan, const char** failed) {
  const hipblasOperation_t opT = HIPBLAS_OP_T, opN = HIPBLAS_OP_N;
  LT_TRY(hipblasLtMatmulDescCreate(&plan->desc, HIPBLAS_COMPUTE_32F,
                                   HIP_R_32F));
  LT_TRY(hipblasLtMatmulDescSetAttribute(
      plan->desc, HIPBLASLT_MATMUL_DESC_TRANSA, &opT, sizeof(opT)));
  LT_TRY(hipblasLtMatmulDescSetAttribute(
      plan->desc, HIPBLASLT_MATMUL_DESC_TRANSB, &opN, sizeof(opN)));
  // column-major views of the row-major operands
  LT_TRY(hipblasLtMatrixLayoutCreate(&plan->la, HIP_R_16BF, K, N, K));  // B
  LT_TRY(hipblasLtMatrixLayoutCreate(&plan->lb, HIP_R_16BF, K, M, K));  // A
  LT_TRY(hipblasLtMatrixLayoutCreate(&plan->lc, HIP_R_16BF, N, M, N));  // C, D
  hipblasLtMatmulPreference_t pref = nullptr;
  LT_TRY(hipblasLtMatmulPreferenceCreate(&pref));
  hipblasStatus_t st = hipblasLtMatmulPreferenceSetAttribute(
      pref, HIPBLASLT_MATMUL_PREF_MAX_WORKSPACE_BYTES, &ws_bytes,
      sizeof(ws_bytes));
  hipblasLtMatmulHeuristicResult_t res = {};
  int found = 0;
  const char* call = "hipblasLtMatmulPreferenceSetAttribute";
  if (st == HIPBLAS_STATUS_SUCCESS) {
    call = "hipblasLtMatmulAlgoGetHeuristic";
    st = hipblasLtMatmulAlgoGetHeuristic(h, plan->desc, plan->la, plan->lb,
                                         plan->lc, plan->lc, pref, 1, &res,
                                         &found);
    if (st == HIPBLAS_STATUS_SUCCESS && found < 1)
      st = HIPBLAS_STATUS_NOT_SUPPORTED;   // no algorithm for this shape
  }
  hipblasLtMatmulPreferenceDestroy(pref);
  if (st != HIPBLAS_STATUS_SUCCESS) {
    *failed = call;
    return (int)st;
  }
  plan->algo = res.algo;
  return 0;
}

void drop_plan(Plan* p) {
  if (p->lc) hipblasLtMatrixLayoutDestroy(p->lc);
  if (p->lb) hipblasLtMatrixLayoutDestroy(p->lb);
  if (p->la) hipblasLtMatrixLayoutDestroy(p->la);
  if (p->desc) hipblasLtMatmulDescDestroy(p->desc);
  *p = Plan();
}

// hipBLASLt encodes its version as major * 100000 + minor * 100 + patch.
constexpr int kHeaderVersion = HIPBLASLT_VERSION_MAJOR * 100000 +
                               HIPBLASLT_VERSION_MINOR * 100 +
                               HIPBLASLT_VERSION_PATCH;

// The device's handle, created on first use; g_mu is held. The structs
// this file passes by layout (hipblasLtMatmulAlgo_t, the heuristic
// result) come from the headers it was compiled with, the code behind
// them from whichever libhipblaslt the process loaded (torch's): a
// library of another major version is refused here, once.
int handle_of(int device, hipblasLtHandle_t* h, const char** failed) {
  auto hit = g_handles.find(device);
  if (hit == g_handles.end()) {
    hipblasLtHandle_t nh = nullptr;
    LT_TRY(hipblasLtCreate(&nh));
    int ver = 0;
    hipblasStatus_t st = hipblasLtGetVersion(nh, &ver);
    if (st == HIPBLAS_STATUS_SUCCESS &&
        ver / 100000 != HIPBLASLT_VERSION_MAJOR)
      st = HIPBLAS_STATUS_NOT_SUPPORTED;
    if (st != HIPBLAS_STATUS_SUCCESS) {
      hipblasLtDestroy(nh);
      *failed = "hipblasLtGetVersion (the loaded library's major version "
                "must be that of the headers)";
      return (int)st;
    }
    g_versions[device] = ver;
    hit = g_handles.emplace(device, nh).first;
  }
  *h = hit->second;
  return 0;
}

}  // namespace

int gemm_nt_add_versions(int device, int* header, int* loaded,
                         const char** failed) {
  std::lock_guard<std::mutex> lock(g_mu);
  hipblasLtHandle_t h;
  const int st = handle_of(device, &h, failed);
  if (st != 0) return st;
  *header = kHeaderVersion;
  *loaded = g_versions[device];
  return 0;
}

int launch_gemm_nt_add(int device, const void* A, const void* B,
                       const void* C, void* D, int M, int N, int K,
                       void* ws, size_t ws_bytes, hipStream_t stream,
                       const char** failed) {
  hipblasLtHandle_t h;
  const Plan* plan;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    const int hst = handle_of(device, &h, failed);
    if (hst != 0) return hst;
    const auto key = std::make_tuple(device, M, N, K);
    auto pit = g_plans.find(key);
    if (pit == g_plans.end()) {
      Plan p;
      const int st = make_plan(h, M, N, K, ws_bytes, &p, failed);
      if (st != 0) {
        drop_plan(&p);
        return st;
      }
      pit = g_plans.emplace(key, p).first;
    }
    plan = &pit->second;      // map nodes never move, plans are never erased
  }
  const float one = 1.0f;
  LT_TRY(hipblasLtMatmul(h, plan->desc, &one, B, plan->la, A, plan->lb, &one,
                         C, plan->lc, D, plan->lc, &plan->algo, ws, ws_bytes,
                         stream));
  return 0;
}
