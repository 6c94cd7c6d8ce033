// Host entry points of the gfx950 kernel library: the one declaration of
// every launcher and planning helper. Host-only (no torch, no device code).
//
// The launchers check nothing. Each comment states what its launcher
// assumes; bindings.cpp is the single gate and enforces it: every pointer
// is device memory of the current device, dense, of the stated type and
// at least the stated element count, and the work is not empty (M, N, B
// >= 1) unless the comment says otherwise. bf16 tensors travel as void*.
#pragma once
#include <hip/hip_runtime_api.h>

// ------------------------------------------------------------ elementwise.hip
// x, y [M,H] bf16, w [H] bf16, inv [M] f32. H % 8 == 0, H <= 16384 (a
// wider row loses its tail).
void launch_rmsnorm_fwd(const void* x, const void* w, void* y, float* inv,
                        int M, int H, float eps, hipStream_t s);
// Grid of the backward = planes of its dw_part workspace.
int rmsnorm_bwd_nblocks(int M);
// dy, x, dx [M,H] bf16; dres [M,H] bf16 or nullptr; inv [M];
// dw_part [rmsnorm_bwd_nblocks(M), H] f32; dw [H] f32. H as in the forward.
void launch_rmsnorm_bwd(const void* dy, const void* x, const void* w,
                        const float* inv, const void* dres, void* dx,
                        float* dw_part, float* dw, int M, int H,
                        hipStream_t s);
// out[L] = sum over the P planes of part [P,L], f32. Any L >= 0, P >= 1.
void launch_reduce_partials(const float* part, float* out, int P, long L,
                            hipStream_t s);
// x, y [B,S,H,D] bf16, D % 8 == 0; cosb, sinb [rows, D/2] f32. Row
// pos0 + s (+ the pos_dev value, - the doc_start offset) is read: pos0 >= 0
// and rows >= pos0 + S without pos_dev, rows >= S with it. pos_dev: one
// int32, or B of them when pos_per_b; its VALUES are the caller's contract
// (pos0 + value + S <= rows). doc_start [B,S] int32 or nullptr (clamped
// in the kernel).
void launch_rope(const void* x, const float* cosb, const float* sinb,
                 void* y, long B, int S, int H, int D, int pos0,
                 int backward, const int* pos_dev, int pos_per_b,
                 const int* doc_start, hipStream_t s);
// g, u, o (and d, dg, du) bf16 with n elements, n % 8 == 0.
void launch_swiglu_fwd(const void* g, const void* u, void* o, long n,
                       hipStream_t s);
void launch_swiglu_bwd(const void* d, const void* g, const void* u,
                       void* dg, void* du, long n, hipStream_t s);

// ------------------------------------------------------------------- xent.hip
// logits, dlogits [N,V] bf16, V % 8 == 0, V > 0; targets [N] int64; loss,
// lse, dloss [N] f32. A target is `ignore` or in [0,V): target VALUES are
// the caller's contract, the kernels index logits with them.
void launch_xent_fwd(const void* logits, const long* targets, float* loss,
                     float* lse, long N, int V, long ignore, hipStream_t s);
void launch_xent_bwd(const void* logits, const long* targets,
                     const float* lse, const float* dloss, void* dlogits,
                     long N, int V, long ignore, hipStream_t s);
// One vocab chunk [N,Vc] that starts at column v0 >= 0; m_run, l_run, tgt,
// lse [N] f32. N >= 1: the grid is min(N, 2048). Vc as V above.
void launch_xent_lse_merge(const void* logits, const long* targets,
                           float* m_run, float* l_run, float* tgt, long N,
                           int Vc, long v0, long ignore_index,
                           hipStream_t s);
void launch_xent_dlogits(const void* logits, const long* targets,
                         const float* lse, void* dl, long N, int Vc,
                         long v0, long ignore_index, hipStream_t s);

// ------------------------------------------------------------------ adamw.hip
// p bf16, master/grad/m/v f32, n elements each, n % 4 == 0. step >= 1
// (step 0 divides by 1 - b^0 = 0).
void launch_adamw(void* p_bf16, float* master, const float* grad, float* m,
                  float* v, long n, float lr, float b1, float b2, float eps,
                  float wd, int step, hipStream_t s);
// x [n] f32, any n >= 0; workspace [1024] f32; out [1] f32.
void launch_l2_norm(const float* x, float* workspace, float* out, long n,
                    hipStream_t s);

// ------------------------------------------------------------------ quant.hip
// q [N,K] int8, scale [N] f32, out [N,K] bf16; K % 8 == 0.
void launch_dequant_int8(const void* q, const float* scale, void* out,
                         long N, int K, hipStream_t s);
// packed [N,K/2] uint8, scale [N,K/group] f32, out [N,K] bf16; K % 8 == 0,
// group % 8 == 0, K % group == 0.
void launch_dequant_int4(const void* packed, const float* scale, void* out,
                         long N, int K, int group, hipStream_t s);

// ------------------------------------------------------------------- lora.hip
// Planning helpers: pure functions of the shape, shared by the launchers
// and the bindings that size the workspaces. K, r >= 1.
int lora_contract_ksplit(int K, long M, int r);   // partial planes; 1 = none
int lora_wgrad_splitm(int K, int r, long M);      // partial planes
// Shapes whose expand-add kernel has an RNG dropout mode; the kernel that
// takes the rest has none, so keep < 1 without a mask is refused there.
bool lora_expand_rng_ok(long M, int N, int r);
// Mk [n] bf16, n % 8 == 0, 0 < keep <= 1.
void launch_dropout_mask(void* Mk, long n, unsigned long long seed,
                         float keep, hipStream_t s);
// X [M,K] bf16, W [r,K] bf16, Mk [M,K] bf16 or nullptr, out [M,r] f32,
// part [lora_contract_ksplit, M, r] f32 (unused when that is 1).
// K % 8 == 0, K >= 8, 1 <= r <= 64, 0 < keep <= 1.
void launch_lora_contract(const void* X, const void* W, const void* Mk,
                          float* part, float* out, long M, int K, int r,
                          unsigned long long seed, float keep,
                          hipStream_t s);
// Two adapters W0, W1 [r,K]: out [2,M,r], part [ksplit,2,M,r]. As above
// with 1 <= r <= 16; no mask tensor.
void launch_lora_contract2(const void* X, const void* W0, const void* W1,
                           float* part, float* out, long M, int K, int r,
                           unsigned long long seed0,
                           unsigned long long seed1, float keep,
                           hipStream_t s);
// Y [M,N] bf16 in place, T [M,r] f32, WT [r,N] bf16, Mk [M,N] bf16 or
// nullptr. N % 8 == 0, r >= 1. keep < 1 without Mk only where
// lora_expand_rng_ok(M, N, r).
void launch_lora_expand_add(void* Y, const float* T, const void* WT,
                            const void* Mk, long M, int N, int r,
                            float scale, unsigned long long seed,
                            float keep, hipStream_t s);
// Two terms, A0/A1 [r,N] bf16, T0/T1 [M,r] f32. N % 8 == 0, 1 <= r <= 16.
void launch_lora_expand_add_dual(void* Y, const float* T0, const float* T1,
                                 const void* A0, const void* A1, long M,
                                 int N, int r, float scale,
                                 unsigned long long seed0,
                                 unsigned long long seed1, float keep,
                                 hipStream_t s);
// T [M,r] f32, X [M,K] bf16, Mk [M,K] bf16 or nullptr, out [r,K] f32,
// part [lora_wgrad_splitm(K, r, M), r, K] f32. K % 8 == 0, r >= 1.
void launch_lora_wgrad(const float* T, const void* X, const void* Mk,
                       float* part, float* out, long M, int K, int r,
                       float s, unsigned long long seed, float keep,
                       hipStream_t st);

// ------------------------------------------------ attn_fwd.hip, attn_bwd.hip
// q, o [B,S,Hq,D], k, v [B,Skv,Hkv,D] bf16, lse [B,Hq,S] f32. D is 64 or
// 128, anything else launches nothing. Hq % Hkv == 0, S, Skv >= 1.
// doc_start [B,S] int32 or nullptr; with it causal, S == Skv, S > 1.
void launch_attn_fwd(const void* q, const void* k, const void* v, void* o,
                     float* lse, const int* doc_start, int B, int Hq,
                     int Hkv, int S, int Skv, int D, float scale,
                     int causal, hipStream_t st);
// x [B,S,H,D] -> xt [B,H,D,S] bf16. D % 64 == 0 (whole 64-column tiles).
void launch_transpose_sd(const void* x, void* xt, int B, int S, int H,
                         int D, hipStream_t st);
// Split-KV chunks of the decode kernel = planes of its part workspace.
int attn_decode_nsplit(int Skv);
// q, o [B,1,Hq,D] bf16; k, v rows of Hkv*D elements, Skv rows per batch
// entry, batch stride Skv*Hkv*D (any stride when B == 1); lse [B,Hq] f32;
// part [B*Hq, attn_decode_nsplit(Skv), D+2] f32. D is 64 or 128, anything
// else launches nothing. len_dev: nullptr, one int32, or B of them when
// len_stride; its VALUES (<= Skv) are the caller's contract.
void launch_attn_decode(const void* q, const void* k, const void* v,
                        const int* len_dev, float* part, void* o,
                        float* lse, int B, int Hq, int Hkv, int Skv,
                        int D, float scale, int len_stride,
                        hipStream_t st);
// Shapes as launch_attn_fwd; dO, dq like q; dk, dv like k; lse, delta
// [B,Hq,S] f32. dq runs first and writes delta, dkdv reads it. D is 64 or
// 128, anything else launches nothing. doc_start / doc_end [B,S] int32,
// both or neither.
void launch_attn_bwd_dq(const void* q, const void* k, const void* v,
                        const void* dO, const void* o, const float* lse,
                        float* delta, void* dq, const int* doc_start,
                        int B, int Hq, int Hkv, int S, int Skv, int D,
                        float scale, int causal, hipStream_t st);
void launch_attn_bwd_dkdv(const void* q, const void* k, const void* v,
                          const void* dO, const float* lse,
                          const float* delta, void* dk, void* dv,
                          const int* doc_end, int B, int Hq, int Hkv,
                          int S, int Skv, int D, float scale, int causal,
                          hipStream_t st);

// ------------------------------------------------------- gemm.hip, gemv.hip
// C[M,N] = A[M,K] @ B[N,K]^T (+ SRC [M,N] or nullptr), bf16.
// N % 256 == 0, K % 64 == 0, K >= 128; any M >= 1.
void launch_gemm_nt(const void* A, const void* B, const void* SRC, void* C,
                    long M, int N, int K, hipStream_t stream);
// y[N] = x[K] @ w[N,K]^T, bf16; K % 8 == 0.
void launch_gemv_bf16(const void* x, const void* w, void* y, int N, int K,
                      hipStream_t st);

// ------------------------------------------------------ qgemv.hip, mlora.hip
// y[M,N] = x[M,K] @ dequant(q)[N,K]^T. 1 <= M <= 16; x, q 16-byte aligned.
// int8: q [N,K], scale [N], K % 16 == 0. int4: packed [N,K/2], scale
// [N,K/group], K % 32 == 0, group % 32 == 0, K % group == 0.
void launch_qgemv_int8(const void* x, const void* q, const float* scale,
                       void* y, int M, int N, int K, hipStream_t st);
void launch_qgemv_int4(const void* x, const void* packed,
                       const float* scale, void* y, int M, int N, int K,
                       int group, hipStream_t st);
// t[m] = x[m] @ a[idx[m]]^T, then y[m] += scale[g] * t[m] @ bt[g]. x [M,K],
// y [M,N] bf16, a [G,R,K], bt [G,R,N] bf16, all 16-byte aligned; t [M,R],
// scale [G] f32; idx [M] int32, a row outside [0,G) is skipped in the
// kernel. 1 <= M <= 16, K % 8 == 0, N % 8 == 0, R in {8, 16, 32, 64}.
void launch_mlora_shrink(const void* x, const void* a, const int* idx,
                         float* t, int M, int K, int R, int G,
                         hipStream_t s);
void launch_mlora_expand_add(void* y, const float* t, const void* bt,
                             const float* scale, const int* idx, int M,
                             int N, int R, int G, hipStream_t s);

// ----------------------------------------------------------------- sample.hip
// Widest row the kernel holds in registers.
long sample_max_vocab();
// logits [B,V] bf16, rows row_stride elements apart (% 8 == 0), 16-byte
// aligned; V % 8 == 0, V <= sample_max_vocab(). temperature, top_p, u f32,
// top_k, offset int32, seed, out int64, B elements each; u may be nullptr.
void launch_sample(const void* logits, long row_stride, int B, int V,
                   const float* temperature, const float* top_p,
                   const int* top_k, const long long* seed,
                   const int* offset, const float* u, long long* out,
                   hipStream_t s);
