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
#include <cstddef>

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
// packed [N,K/2] uint8 (NF4 level indices), absmax [N,K/group] f32, out
// [N,K] bf16 (16-byte aligned); K % 8 == 0, group % 8 == 0, K % group == 0.
void launch_dequant_nf4(const void* packed, const float* absmax, void* out,
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
// The second half of launch_attn_decode alone: part [BH, NS, D+2] f32 ->
// o [BH, D] bf16, lse [BH] f32. D is 64 or 128, NS >= 1.
void launch_attn_decode_combine(const float* part, void* o, float* lse,
                                int BH, int NS, int D, hipStream_t st);

// -------------------------------------------------------- attn_decode_gqa.hip
// Head shapes the GQA-shared bf16 decode kernel takes: D in {64, 128},
// Hq % Hkv == 0 and a group of 2 .. 16 query heads per kv head. The one
// predicate: the binding checks it and Python routes by it.
bool gqa_decode_supported(int Hq, int Hkv, int D);
// Split plan: rows per chunk (a multiple of 128) and chunks (at most 32) =
// planes of the part workspace. A function of the addressed capacity and
// the head shape alone, never of B or of the live lengths.
int attn_decode_gqa_chunk(int Skv, int Hkv, int D);
int attn_decode_gqa_nsplit(int Skv, int Hkv, int D);
// As launch_attn_decode, one block per KV head and chunk: q, o [B,1,Hq,D]
// bf16; k, v rows of Hkv*D elements, Skv rows per batch entry, batch stride
// Skv*Hkv*D (any stride when B == 1); q, k, v 16-byte aligned; lse [B,Hq]
// f32; part [B*Hq, attn_decode_gqa_nsplit(Skv, Hkv, D), D+2] f32.
// gqa_decode_supported(Hq, Hkv, D), Skv >= 1. len_dev: nullptr (all Skv
// rows live), one int32, or B of them when len_stride; read on the device
// and clamped to Skv there, <= 0 gives o = 0.
void launch_attn_decode_gqa(const void* q, const void* k, const void* v,
                            const int* len_dev, float* part, void* o,
                            float* lse, int B, int Hq, int Hkv, int Skv,
                            int D, float scale, int len_stride,
                            hipStream_t st);

// ------------------------------------------------------------ attn_verify.hip
// Shapes the multi-token verify kernel takes: D in {64, 128}, Hq % Hkv ==
// 0, 1 <= T <= 16 query rows a sequence and T * (Hq / Hkv) <= 32 MFMA
// columns a kv head. The one predicate: the binding checks it and Python
// routes by it.
bool attn_verify_supported(int T, int Hq, int Hkv, int D);
// Split plan (attn_decode_gqa's): rows per chunk and chunks = planes of the
// part workspace; a function of the addressed capacity and the head shape.
int attn_verify_chunk(int Skv, int Hkv, int D);
int attn_verify_nsplit(int Skv, int Hkv, int D);
// q, o [B,T,Hq,D] bf16; k, v as launch_attn_decode_gqa, holding the T new
// rows already; lse [B,T,Hq] f32; part [B*T*Hq, attn_verify_nsplit(Skv,
// Hkv, D), D+2] f32. attn_verify_supported(T, Hq, Hkv, D), Skv >= 1.
// len_dev: nullptr (all Skv rows live), one int32, or B of them when
// len_stride: the live length INCLUDING the T rows, read on the device and
// clamped to Skv there. Query t sees rows j <= len - T + t; a query with a
// negative limit (len < T) gets o = 0.
void launch_attn_verify(const void* q, const void* k, const void* v,
                        const int* len_dev, float* part, void* o,
                        float* lse, int B, int T, int Hq, int Hkv, int Skv,
                        int D, float scale, int len_stride,
                        hipStream_t st);

// -------------------------------------------------------------------- kvq.hip
// int8 KV cache: k8, v8 [Bc, max_s, Hkv, D] int8, ks, vs [Bc, Hkv, max_s]
// f32 (one scale per token and kv head). D is 64 or 128, anything else
// launches nothing.
// k, v [B,S,Hkv,D] bf16, quantized row by row into the cache; k, v, k8, v8
// 16-byte aligned. Without wpos row (b, s) goes to slot (b, start + s):
// B <= Bc, 0 <= start, start + S <= max_s. With wpos (int64 [B], S == 1)
// row b goes to the flat slot wpos[b] of [Bc * max_s]; a value outside
// that range is skipped in the kernel.
void launch_kv_quant_append(const void* k, const void* v, void* k8,
                            void* v8, float* ks, float* vs,
                            const long long* wpos, long B, int S, int Hkv,
                            int D, long Bc, int max_s, int start,
                            hipStream_t st);
// Split plan of the decode kernel: rows per chunk (a multiple of 128) and
// chunks = planes of its part workspace. A function of the capacity and
// the head shape alone, never of B or of the live lengths.
int attn_decode_q8_chunk(int max_s, int Hkv, int D);
int attn_decode_q8_nsplit(int max_s, int Hkv, int D);
// q, o [B,1,Hq,D] bf16, q, k8, v8 16-byte aligned; B <= Bc; lse [B,Hq] f32;
// part [B*Hq, attn_decode_q8_nsplit(max_s, Hkv, D), D+2] f32.
// Hq % Hkv == 0 and 1 <= Hq / Hkv <= 16. Live rows of batch row b: len_dev
// (one int32, or B of them when len_stride) read on the device, else
// `length`; either is clamped to max_s in the kernel, <= 0 gives o = 0.
void launch_attn_decode_q8(const void* q, const void* k8, const void* v8,
                           const float* ks, const float* vs,
                           const int* len_dev, int length, float* part,
                           void* o, float* lse, int B, int Hq, int Hkv,
                           int max_s, int D, float scale, int len_stride,
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

// ------------------------------------------- gemm.hip, gemm_fp8.hip, gemv.hip
// C[M,N] = A[M,K] @ B[N,K]^T (+ SRC [M,N] or nullptr), bf16.
// N % 256 == 0, K % 64 == 0, K >= 128; any M >= 1.
void launch_gemm_nt(const void* A, const void* B, const void* SRC, void* C,
                    long M, int N, int K, hipStream_t stream);
// gemm_fp8.hip: x [M,K] bf16 -> q [M,K] e4m3 (one byte each), scale [M]
// f32 with scale = absmax(row) / 448 (1 for a zero row) and q =
// e4m3_rne(clamp(x / scale, -448, 448)). K % 8 == 0, 8 <= K <=
// quant_fp8_max_k() (a row is held in registers); x, q 16-byte aligned.
long quant_fp8_max_k();
void launch_quant_fp8_rows(const void* x, void* q, float* scale, long M,
                           int K, hipStream_t st);
// Shapes the fp8 GEMM takes: N % 256 == 0, K % 128 == 0, 256 <= K <= 2^23.
// The one predicate: the binding checks it and Python routes by it.
bool gemm_fp8_supported(long N, long K);
// C[M,N] bf16 = SA[m] * SB[n] * sum_k A[m,k] * B[n,k] (+ SRC [M,N] bf16 or
// nullptr); A [M,K], B [N,K] e4m3, SA [M], SB [N] f32. All 16-byte aligned,
// gemm_fp8_supported(N, K), any M >= 1.
void launch_gemm_fp8_nt(const void* A, const float* SA, const void* B,
                        const float* SB, const void* SRC, void* C, long M,
                        int N, int K, hipStream_t stream);
// basegemm.cpp, on hipBLASLt: D[M,N] = A[M,K] @ B[N,K]^T + C[M,N], bf16,
// fp32 accumulate; C is only read, D != C. All four 16-byte aligned,
// M, N, K >= 1. ws: ws_bytes of device scratch the call may use until it
// has run on `stream`. `device` is the current device (it keys the handle
// and the per-shape plans). Returns 0, or the hipBLASLt status with
// *failed naming the call that gave it.
int launch_gemm_nt_add(int device, const void* A, const void* B,
                       const void* C, void* D, int M, int N, int K,
                       void* ws, size_t ws_bytes, hipStream_t stream,
                       const char** failed);
// hipBLASLt versions (major * 100000 + minor * 100 + patch): of the headers
// basegemm.cpp was compiled with, and of the library the process loaded.
// Creates the device's handle if need be; returns as launch_gemm_nt_add.
int gemm_nt_add_versions(int device, int* header, int* loaded,
                         const char** failed);
// y[N] = x[K] @ w[N,K]^T, bf16; K % 8 == 0.
void launch_gemv_bf16(const void* x, const void* w, void* y, int N, int K,
                      hipStream_t st);

// ----------------------------------------------------------------- skinny.hip
// Shapes the bf16 weight-streaming kernels take and win at: 1 <= M <= 16,
// N >= 1, K >= 8, K % 8 == 0, K <= 2^24, and M <= 2 where N >= 16384 (the
// library ties or wins there). The one predicate of the family: the
// bindings check it and Python routes by it.
bool skinny_supported(long M, long N, long K);
// y[i][M,N[i]] = x[M,K] @ w[i][N[i],K]^T for nw in 1..3 weights in one
// grid, bf16; + residual [M,N[0]] (or nullptr) when nw == 1. x and every
// w[i] 16-byte aligned, skinny_supported(M, N[i], K). The grid and an
// output's summation order depend on (N[i], K) alone: each y[i] has the
// bits of its single-weight launch, a row's bits do not depend on M.
void launch_skinny_gemm(const void* x, const void* const* w,
                        const void* residual, void* const* y, const int* N,
                        int nw, int M, int K, hipStream_t st);
// y[M,N] = swiglu(bf16(x @ wg^T), bf16(x @ wu^T)); wg, wu [N,K]. As above.
void launch_skinny_swiglu(const void* x, const void* wg, const void* wu,
                          void* y, int M, int N, int K, hipStream_t st);

// ------------------------------------------------------ qgemv.hip, mlora.hip
// y[M,N] = x[M,K] @ dequant(q)[N,K]^T. 1 <= M <= 16; x, q 16-byte aligned.
// int8: q [N,K], scale [N], K % 16 == 0. int4: packed [N,K/2], scale
// [N,K/group], K % 32 == 0, group % 32 == 0, K % group == 0.
void launch_qgemv_int8(const void* x, const void* q, const float* scale,
                       void* y, int M, int N, int K, hipStream_t st);
void launch_qgemv_int4(const void* x, const void* packed,
                       const float* scale, void* y, int M, int N, int K,
                       int group, hipStream_t st);
// qgemv_nf4.hip: the int4 contract with NF4 level indices in the nibbles
// and the group's absmax as its scale.
void launch_qgemv_nf4(const void* x, const void* packed, const float* absmax,
                      void* y, int M, int N, int K, int group,
                      hipStream_t st);
// qgemv_fp8.hip: shapes the e4m3 weight-streaming kernel takes: 1 <= M <=
// 16, N >= 1, K % 128 == 0, 128 <= K <= quant_fp8_max_k(). The one
// predicate: the binding checks it and Python routes by it.
bool qgemv_fp8_supported(long M, long N, long K);
// y[M,N] bf16 = sa[m] * sw[n] * sum_k x8[m,k] * w8[n,k] with (x8, sa) =
// quant_fp8_rows(x) formed in the kernel; x [M,K] bf16, w8 [N,K] e4m3, both
// 16-byte aligned, sw [N] f32. qgemv_fp8_supported(M, N, K). The grid and
// an output's summation order depend on (N, K) alone: a row's bits do not
// depend on M.
void launch_qgemv_fp8(const void* x, const void* w8, const float* sw,
                      void* y, int M, int N, int K, hipStream_t st);
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
