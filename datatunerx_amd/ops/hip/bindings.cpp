// Torch bindings for the gfx950 HIP kernel library.
// All tensors must be contiguous; bf16 compute dtype, fp32 reductions.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>

// ---- launchers (defined in the .hip files) ----
void launch_rmsnorm_fwd(const void*, const void*, void*, float*, int, int,
                        float, hipStream_t);
int rmsnorm_bwd_nblocks(int M);
void launch_rmsnorm_bwd(const void*, const void*, const void*, const float*,
                        const void*, void*, float*, float*, int, int,
                        hipStream_t);
void launch_rope(const void*, const float*, const float*, void*, long, int,
                 int, int, int, int, const int*, int, const int*,
                 hipStream_t);
void launch_swiglu_fwd(const void*, const void*, void*, long, hipStream_t);
void launch_swiglu_bwd(const void*, const void*, const void*, void*, void*,
                       long, hipStream_t);
void launch_xent_fwd(const void*, const long*, float*, float*, long, int,
                     long, hipStream_t);
void launch_xent_bwd(const void*, const long*, const float*, const float*,
                     void*, long, int, long, hipStream_t);
void launch_dequant_int8(const void*, const float*, void*, long, int,
                         hipStream_t);
void launch_dequant_int4(const void*, const float*, void*, long, int, int,
                         hipStream_t);
void launch_xent_lse_merge(const void*, const long*, float*, float*,
                           float*, long, int, long, long, hipStream_t);
void launch_xent_dlogits(const void*, const long*, const float*, void*,
                         long, int, long, long, hipStream_t);
void launch_adamw(void*, float*, const float*, float*, float*, long, float,
                  float, float, float, float, int, hipStream_t);
void launch_l2_norm(const float*, float*, float*, long, hipStream_t);
int lora_contract_ksplit(int K, long M, int r);
void launch_dropout_mask(void*, long, unsigned long long, float,
                         hipStream_t);
void launch_lora_contract(const void*, const void*, const void*, float*,
                          float*, long, int, int, unsigned long long,
                          float, hipStream_t);
void launch_lora_expand_add(void*, const float*, const void*, const void*,
                            long, int, int, float, unsigned long long,
                            float, hipStream_t);
bool lora_expand_rng_ok(long M, int N, int r);
int lora_wgrad_splitm(int K, int r, long M);
void launch_lora_contract2(const void*, const void*, const void*, float*,
                           float*, long, int, int, unsigned long long,
                           unsigned long long, float, hipStream_t);
void launch_lora_expand_add_dual(void*, const float*, const float*,
                                 const void*, const void*, long, int, int,
                                 float, unsigned long long,
                                 unsigned long long, float, hipStream_t);
void launch_lora_wgrad(const float*, const void*, const void*, float*,
                       float*, long, int, int, float, unsigned long long,
                       float, hipStream_t);
void launch_attn_fwd(const void*, const void*, const void*, void*, float*,
                     const int*, int, int, int, int, int, int, float, int,
                     hipStream_t);
void launch_transpose_sd(const void*, void*, int, int, int, int,
                         hipStream_t);
int attn_decode_nsplit(int Skv);
void launch_gemv_bf16(const void*, const void*, void*, int, int,
                      hipStream_t);
void launch_qgemv_int8(const void*, const void*, const float*, void*, int,
                       int, int, hipStream_t);
void launch_qgemv_int4(const void*, const void*, const float*, void*, int,
                       int, int, int, hipStream_t);
void launch_mlora_shrink(const void*, const void*, const int*, float*, int,
                         int, int, int, hipStream_t);
void launch_mlora_expand_add(void*, const float*, const void*, const float*,
                             const int*, int, int, int, int, hipStream_t);
void launch_gemm_nt(const void*, const void*, const void*, void*, long,
                    int, int, hipStream_t);
long sample_max_vocab();
void launch_sample(const void*, long, int, int, const float*, const float*,
                   const int*, const long long*, const int*, const float*,
                   long long*, hipStream_t);
void launch_attn_decode(const void*, const void*, const void*,
                        const int*, float*, void*, float*, int, int, int,
                        int, int, float, int, hipStream_t);
void launch_attn_bwd_dkdv(const void*, const void*, const void*,
                          const void*, const float*, const float*,
                          void*, void*, const int*, int, int, int, int,
                          int, int, float, int, hipStream_t);
void launch_attn_bwd_dq(const void*, const void*, const void*,
                        const void*, const void*, const float*, float*,
                        void*, const int*, int, int, int, int, int, int,
                        float, int, hipStream_t);

namespace {

hipStream_t cur_stream() {
  return (hipStream_t)at::cuda::getCurrentCUDAStream().stream();
}

void check_bf16_contig(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// Sequence-packing maps (doc_start / doc_end): int32 [B,S] on the GPU.
// The kernels index them unchecked, so shape and layout are pinned here.
const int* doc_map_ptr(const c10::optional<torch::Tensor>& t, long B,
                       long S, const char* name) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK(t->is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t->scalar_type() == torch::kInt, name, " must be int32");
  TORCH_CHECK(t->dim() == 2 && t->size(0) == B && t->size(1) == S, name,
              " must be [B,S]");
  TORCH_CHECK(t->is_contiguous(), name, " must be contiguous");
  return t->data_ptr<int>();
}

// doc_start needs the training shape: causal self-attention over S > 1.
void check_docs_shape(bool causal, long S, long Skv) {
  TORCH_CHECK(causal, "doc_start requires causal=True");
  TORCH_CHECK(S == Skv, "doc_start requires S == Skv");
  TORCH_CHECK(S > 1, "doc_start requires S > 1");
}

// ------------------------------------------------------------- RMSNorm
// The kernels hold one row in registers, at most 8 groups of 8 columns per
// thread: H <= 8 * 8 * 256. A wider row would lose its tail silently.
constexpr long RMSNORM_MAX_H = 8L * 8 * 256;

void check_rmsnorm_row(const torch::Tensor& x, const torch::Tensor& w) {
  check_bf16_contig(x, "x");
  check_bf16_contig(w, "w");
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) > 0, "x must be [..., H]");
  const long H = x.size(-1);
  TORCH_CHECK(H % 8 == 0, "H % 8");
  TORCH_CHECK(H <= RMSNORM_MAX_H, "rmsnorm: H = ", H,
              " is above the kernel limit of ", RMSNORM_MAX_H);
  TORCH_CHECK(w.numel() == H, "w must have H elements");
}

std::vector<torch::Tensor> rmsnorm_fwd(torch::Tensor x, torch::Tensor w,
                                       double eps) {
  check_rmsnorm_row(x, w);
  const int H = (int)x.size(-1);
  const long M = x.numel() / H;
  auto y = torch::empty_like(x);
  auto inv = torch::empty({M}, x.options().dtype(torch::kFloat));
  launch_rmsnorm_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(),
                     inv.data_ptr<float>(), (int)M, H, (float)eps,
                     cur_stream());
  return {y, inv};
}

std::vector<torch::Tensor> rmsnorm_bwd(torch::Tensor dy, torch::Tensor x,
                                       torch::Tensor w, torch::Tensor inv,
                                       c10::optional<torch::Tensor> dres) {
  check_bf16_contig(dy, "dy");
  check_rmsnorm_row(x, w);
  const int H = (int)x.size(-1);
  const long M = x.numel() / H;
  TORCH_CHECK(dy.sizes() == x.sizes(), "dy must have the shape of x");
  TORCH_CHECK(inv.is_cuda() && inv.scalar_type() == torch::kFloat &&
              inv.is_contiguous() && inv.numel() == M,
              "inv must be contiguous f32 on GPU with one element per row");
  auto dx = torch::empty_like(x);
  auto dw = torch::empty({H}, x.options().dtype(torch::kFloat));
  const int nb = rmsnorm_bwd_nblocks((int)M);
  auto part = torch::empty({nb, H}, x.options().dtype(torch::kFloat));
  const void* drp = nullptr;
  if (dres.has_value()) {
    check_bf16_contig(*dres, "dres");
    TORCH_CHECK(dres->numel() == x.numel(), "dres shape");
    drp = dres->data_ptr();
  }
  launch_rmsnorm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(),
                     inv.data_ptr<float>(), drp, dx.data_ptr(),
                     part.data_ptr<float>(), dw.data_ptr<float>(), (int)M, H,
                     cur_stream());
  return {dx, dw};
}

// ---------------------------------------------------------------- RoPE
torch::Tensor rope(torch::Tensor x, torch::Tensor cosb, torch::Tensor sinb,
                   long pos0, bool backward,
                   c10::optional<torch::Tensor> pos_dev,
                   c10::optional<torch::Tensor> doc_start) {
  check_bf16_contig(x, "x");
  TORCH_CHECK(x.dim() == 4, "x must be [B,S,H,D]");
  TORCH_CHECK(cosb.scalar_type() == torch::kFloat && cosb.is_contiguous());
  const int B = (int)x.size(0), S = (int)x.size(1), H = (int)x.size(2),
            D = (int)x.size(3);
  TORCH_CHECK(D % 8 == 0, "D % 8");
  const int* dsp = doc_map_ptr(doc_start, B, S, "doc_start");
  TORCH_CHECK(!(dsp && pos_dev.has_value()),
              "doc_start cannot be combined with pos_dev");
  const int* pd = nullptr;
  int pos_per_b = 0;
  if (pos_dev.has_value()) {
    TORCH_CHECK(pos_dev->scalar_type() == torch::kInt &&
                pos_dev->is_cuda(), "pos_dev must be int32 on GPU");
    pd = pos_dev->data_ptr<int>();
    pos_per_b = pos_dev->numel() > 1;
    if (pos_per_b)
      TORCH_CHECK(pos_dev->numel() == B, "pos_dev must be [1] or [B]");
    TORCH_CHECK(cosb.size(0) >= S, "rope table too short");
  } else {
    TORCH_CHECK(cosb.size(0) >= pos0 + S, "rope table too short");
  }
  auto y = torch::empty_like(x);
  launch_rope(x.data_ptr(), cosb.data_ptr<float>(), sinb.data_ptr<float>(),
              y.data_ptr(), B, S, H, D, (int)pos0, backward ? 1 : 0, pd,
              pos_per_b, dsp, cur_stream());
  return y;
}

// --------------------------------------------------------------- SwiGLU
torch::Tensor swiglu_fwd(torch::Tensor gate, torch::Tensor up) {
  check_bf16_contig(gate, "gate");
  check_bf16_contig(up, "up");
  TORCH_CHECK(gate.numel() % 8 == 0);
  auto out = torch::empty_like(gate);
  launch_swiglu_fwd(gate.data_ptr(), up.data_ptr(), out.data_ptr(),
                    gate.numel(), cur_stream());
  return out;
}

std::vector<torch::Tensor> swiglu_bwd(torch::Tensor dout, torch::Tensor gate,
                                      torch::Tensor up) {
  check_bf16_contig(dout, "dout");
  check_bf16_contig(gate, "gate");
  check_bf16_contig(up, "up");
  TORCH_CHECK(gate.numel() % 8 == 0);
  TORCH_CHECK(up.sizes() == gate.sizes() && dout.sizes() == gate.sizes(),
              "dout, gate and up must have one shape");
  auto dg = torch::empty_like(gate);
  auto du = torch::empty_like(up);
  launch_swiglu_bwd(dout.data_ptr(), gate.data_ptr(), up.data_ptr(),
                    dg.data_ptr(), du.data_ptr(), gate.numel(),
                    cur_stream());
  return {dg, du};
}

// -------------------------------------------------------- cross entropy
std::vector<torch::Tensor> xent_fwd(torch::Tensor logits,
                                    torch::Tensor targets, long ignore) {
  check_bf16_contig(logits, "logits");
  TORCH_CHECK(targets.scalar_type() == torch::kLong);
  const int V = (int)logits.size(-1);
  const long N = logits.numel() / V;
  TORCH_CHECK(V % 8 == 0, "V % 8");
  auto loss = torch::empty({N}, logits.options().dtype(torch::kFloat));
  auto lse = torch::empty({N}, logits.options().dtype(torch::kFloat));
  launch_xent_fwd(logits.data_ptr(), targets.data_ptr<long>(),
                  loss.data_ptr<float>(), lse.data_ptr<float>(), N, V,
                  ignore, cur_stream());
  return {loss, lse};
}

torch::Tensor xent_bwd(torch::Tensor logits, torch::Tensor targets,
                       torch::Tensor lse, torch::Tensor dloss, long ignore) {
  check_bf16_contig(logits, "logits");
  const int V = (int)logits.size(-1);
  const long N = logits.numel() / V;
  auto dlogits = torch::empty_like(logits);
  launch_xent_bwd(logits.data_ptr(), targets.data_ptr<long>(),
                  lse.data_ptr<float>(), dloss.data_ptr<float>(),
                  dlogits.data_ptr(), N, V, ignore, cur_stream());
  return dlogits;
}

// ----------------------------------------------------------------- LoRA
// Optional `mask` (bf16, same shape as x / y) fuses the PEFT-style
// input dropout into the kernels (no mask-multiply materialization).
static const void* opt_mask(const c10::optional<torch::Tensor>& m,
                            long numel, const char* name) {
  if (!m.has_value()) return nullptr;
  check_bf16_contig(*m, name);
  TORCH_CHECK(m->numel() == numel, name, " shape mismatch");
  return m->data_ptr();
}

torch::Tensor lora_contract(torch::Tensor x, torch::Tensor w,
                            c10::optional<torch::Tensor> mask,
                            int64_t seed, double keep) {
  check_bf16_contig(x, "x");
  check_bf16_contig(w, "w");
  const int K = (int)x.size(-1);
  const long M = x.numel() / K;
  const int r = (int)w.size(0);
  TORCH_CHECK(w.size(1) == K, "w [r,K] mismatch");
  TORCH_CHECK(r <= 64, "r <= 64");
  TORCH_CHECK(K % 8 == 0);
  auto t = torch::empty({M, r}, x.options().dtype(torch::kFloat));
  const int nsplit = lora_contract_ksplit(K, M, r);
  torch::Tensor part;
  float* part_ptr = nullptr;
  if (nsplit > 1) {
    part = torch::empty({nsplit, M, r}, x.options().dtype(torch::kFloat));
    part_ptr = part.data_ptr<float>();
  }
  launch_lora_contract(x.data_ptr(), w.data_ptr(),
                       opt_mask(mask, x.numel(), "mask"), part_ptr,
                       t.data_ptr<float>(), M, K, r,
                       (unsigned long long)seed, (float)keep,
                       cur_stream());
  return t;
}

// Two adapters, two dropout seeds, one pass over x: (t0, t1), each
// bit-identical to lora_contract with its own adapter and seed.
std::vector<torch::Tensor> lora_contract2(torch::Tensor x, torch::Tensor w0,
                                          torch::Tensor w1, int64_t seed0,
                                          int64_t seed1, double keep) {
  check_bf16_contig(x, "x");
  check_bf16_contig(w0, "w0");
  check_bf16_contig(w1, "w1");
  const int K = (int)x.size(-1);
  const long M = x.numel() / K;
  const int r = (int)w0.size(0);
  TORCH_CHECK(w0.dim() == 2 && w0.sizes() == w1.sizes() && w0.size(1) == K,
              "w0/w1 [r,K] mismatch");
  TORCH_CHECK(r >= 1 && r <= 16, "lora_contract2: r <= 16");
  TORCH_CHECK(K % 8 == 0);
  auto t = torch::empty({2, M, r}, x.options().dtype(torch::kFloat));
  const int nsplit = lora_contract_ksplit(K, M, r);
  torch::Tensor part;
  float* part_ptr = nullptr;
  if (nsplit > 1) {
    part = torch::empty({nsplit, 2, M, r},
                        x.options().dtype(torch::kFloat));
    part_ptr = part.data_ptr<float>();
  }
  launch_lora_contract2(x.data_ptr(), w0.data_ptr(), w1.data_ptr(),
                        part_ptr, t.data_ptr<float>(), M, K, r,
                        (unsigned long long)seed0,
                        (unsigned long long)seed1, (float)keep,
                        cur_stream());
  return {t[0], t[1]};
}

// wt is the adapter already in [r,N] (lora_B transposed, or lora_A as it
// is for the dx term): no transposed copy per call.
void lora_expand_add_t(torch::Tensor y, torch::Tensor t, torch::Tensor wt,
                       double scale, c10::optional<torch::Tensor> mask,
                       int64_t seed, double keep) {
  check_bf16_contig(y, "y");
  check_bf16_contig(wt, "wt");
  const int N = (int)y.size(-1);
  const long M = y.numel() / N;
  const int r = (int)wt.size(0);
  TORCH_CHECK(wt.dim() == 2 && wt.size(1) == N, "wt [r,N] mismatch");
  TORCH_CHECK(t.scalar_type() == torch::kFloat && t.is_contiguous() &&
              t.numel() == M * r, "t [M,r] f32");
  TORCH_CHECK(keep >= 1.0 || lora_expand_rng_ok(M, N, r),
              "RNG dropout needs the r<=16 fast path; materialize the "
              "mask for this shape");
  launch_lora_expand_add(y.data_ptr(), t.data_ptr<float>(), wt.data_ptr(),
                         opt_mask(mask, y.numel(), "mask"), M, N, r,
                         (float)scale, (unsigned long long)seed,
                         (float)keep, cur_stream());
}

// y += mask0 o (s * t0 @ a0) + mask1 o (s * t1 @ a1), a0/a1 [r,N]: one
// read-modify-write of y, one rounding.
void lora_expand_add2(torch::Tensor y, torch::Tensor t0, torch::Tensor t1,
                      torch::Tensor a0, torch::Tensor a1, double scale,
                      int64_t seed0, int64_t seed1, double keep) {
  check_bf16_contig(y, "y");
  check_bf16_contig(a0, "a0");
  check_bf16_contig(a1, "a1");
  const int N = (int)y.size(-1);
  const long M = y.numel() / N;
  const int r = (int)a0.size(0);
  TORCH_CHECK(a0.dim() == 2 && a0.sizes() == a1.sizes() && a0.size(1) == N,
              "a0/a1 [r,N] mismatch");
  TORCH_CHECK(r >= 1 && r <= 16 && N % 8 == 0,
              "lora_expand_add2: r <= 16, N % 8 == 0");
  for (const auto& t : {t0, t1})
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat &&
                t.is_contiguous() && t.numel() == M * r, "t [M,r] f32");
  if (M == 0) return;
  launch_lora_expand_add_dual(y.data_ptr(), t0.data_ptr<float>(),
                              t1.data_ptr<float>(), a0.data_ptr(),
                              a1.data_ptr(), M, N, r, (float)scale,
                              (unsigned long long)seed0,
                              (unsigned long long)seed1, (float)keep,
                              cur_stream());
}

torch::Tensor lora_wgrad(torch::Tensor t, torch::Tensor x, double scale,
                         c10::optional<torch::Tensor> mask,
                         int64_t seed, double keep) {
  check_bf16_contig(x, "x");
  TORCH_CHECK(t.scalar_type() == torch::kFloat && t.is_contiguous());
  const int K = (int)x.size(-1);
  const long M = x.numel() / K;
  const int r = (int)t.size(-1);
  auto out = torch::empty({r, K}, x.options().dtype(torch::kFloat));
  const int sm = lora_wgrad_splitm(K, r, M);
  auto part = torch::empty({sm, r, K}, x.options().dtype(torch::kFloat));
  launch_lora_wgrad(t.data_ptr<float>(), x.data_ptr(),
                    opt_mask(mask, x.numel(), "mask"),
                    part.data_ptr<float>(), out.data_ptr<float>(), M, K, r,
                    (float)scale, (unsigned long long)seed, (float)keep,
                    cur_stream());
  return out;
}

// Materialize the RNG dropout mask (bit-identical to what the fused
// MODE==2 kernels consume) — used by tests and the r>16 fallback.
torch::Tensor dropout_mask(int64_t M, int64_t K, int64_t seed, double keep,
                           torch::Tensor like) {
  TORCH_CHECK((M * K) % 8 == 0, "M*K % 8 == 0");
  auto m = torch::empty({M, K}, like.options().dtype(torch::kBFloat16));
  launch_dropout_mask(m.data_ptr(), M * K, (unsigned long long)seed,
                      (float)keep, cur_stream());
  return m;
}

// ---------------------------------------------------------------- AdamW
void adamw(torch::Tensor p, torch::Tensor master, torch::Tensor grad,
           torch::Tensor m, torch::Tensor v, double lr, double b1, double b2,
           double eps, double wd, long step) {
  check_bf16_contig(p, "p");
  TORCH_CHECK(master.scalar_type() == torch::kFloat);
  TORCH_CHECK(grad.scalar_type() == torch::kFloat);
  TORCH_CHECK(p.numel() % 4 == 0, "flat param buffer must be padded to 4");
  launch_adamw(p.data_ptr(), master.data_ptr<float>(),
               grad.data_ptr<float>(), m.data_ptr<float>(),
               v.data_ptr<float>(), p.numel(), (float)lr, (float)b1,
               (float)b2, (float)eps, (float)wd, (int)step, cur_stream());
}

torch::Tensor l2_norm(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kFloat &&
              x.is_contiguous());
  auto ws = torch::empty({1024}, x.options());
  auto out = torch::empty({1}, x.options());
  launch_l2_norm(x.data_ptr<float>(), ws.data_ptr<float>(),
                 out.data_ptr<float>(), x.numel(), cur_stream());
  return out;
}

// ------------------------------------------------------------ attention
// [B,S,H,D] -> [B,H,D,S]
torch::Tensor transpose_sd(torch::Tensor x) {
  check_bf16_contig(x, "x");
  TORCH_CHECK(x.dim() == 4, "x must be [B,S,H,D]");
  const int B = (int)x.size(0), S = (int)x.size(1), H = (int)x.size(2),
            D = (int)x.size(3);
  auto xt = torch::empty({B, H, D, S}, x.options());
  launch_transpose_sd(x.data_ptr(), xt.data_ptr(), B, S, H, D,
                      cur_stream());
  return xt;
}

// q: [B,S,Hq,D]; k, v: [B,Skv,Hkv,D] — all BSHD, v row-major like k.
std::vector<torch::Tensor> attn_fwd(torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, bool causal,
                                    double scale,
                                    c10::optional<torch::Tensor> doc_start) {
  check_bf16_contig(q, "q");
  check_bf16_contig(k, "k");
  check_bf16_contig(v, "v");
  const int B = (int)q.size(0), S = (int)q.size(1), Hq = (int)q.size(2),
            D = (int)q.size(3);
  const int Skv = (int)k.size(1), Hkv = (int)k.size(2);
  TORCH_CHECK(v.size(1) == Skv && v.size(2) == Hkv && v.size(3) == D,
              "v must be BSHD like k");
  TORCH_CHECK(D == 64 || D == 128, "D must be 64 or 128");
  TORCH_CHECK(Hq % Hkv == 0, "GQA group");
  const int* dsp = doc_map_ptr(doc_start, B, S, "doc_start");
  if (dsp) check_docs_shape(causal, S, Skv);
  auto o = torch::empty_like(q);
  auto lse = torch::empty({B, Hq, S}, q.options().dtype(torch::kFloat));
  launch_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                  lse.data_ptr<float>(), dsp, B, Hq, Hkv, S, Skv, D,
                  (float)scale, causal ? 1 : 0, cur_stream());
  return {o, lse};
}

// C[M,N] = A[M,K] @ B[N,K]^T (+ optional bf16 src) — the hand-written
// 256x256-tile MFMA GEMM (gemm.hip). Requires N % 256 == 0, K % 64 == 0,
// K >= 128; any M (SRSRC-clamped tail).
torch::Tensor gemm_nt(torch::Tensor a, torch::Tensor b,
                      c10::optional<torch::Tensor> src) {
  check_bf16_contig(a, "a");
  check_bf16_contig(b, "b");
  const int K = (int)b.size(1), N = (int)b.size(0);
  const long M = a.numel() / K;
  TORCH_CHECK(a.size(-1) == K, "gemm_nt: inner dims");
  TORCH_CHECK(N % 256 == 0 && K % 64 == 0 && K >= 128,
              "gemm_nt: unsupported shape N=", N, " K=", K);
  auto sizes = a.sizes().vec();
  sizes[sizes.size() - 1] = N;
  auto c = torch::empty(sizes, a.options());
  const void* sp = nullptr;
  if (src.has_value()) {
    check_bf16_contig(*src, "src");
    TORCH_CHECK(src->numel() == M * N, "gemm_nt: src shape");
    sp = src->data_ptr();
  }
  launch_gemm_nt(a.data_ptr(), b.data_ptr(), sp, c.data_ptr(), M, N, K,
                 cur_stream());
  return c;
}

// weight-only dequant (int8 per-row / int4 group-64) -> bf16
torch::Tensor dequant_int8(torch::Tensor q, torch::Tensor scale) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == torch::kChar &&
              q.is_contiguous());
  const int K = (int)q.size(1);
  const long N = q.size(0);
  TORCH_CHECK(K % 8 == 0, "K % 8");
  auto out = torch::empty({N, K},
                          q.options().dtype(torch::kBFloat16));
  launch_dequant_int8(q.data_ptr(), scale.data_ptr<float>(),
                      out.data_ptr(), N, K, cur_stream());
  return out;
}

torch::Tensor dequant_int4(torch::Tensor packed, torch::Tensor scale,
                           long group) {
  TORCH_CHECK(packed.is_cuda() && packed.scalar_type() == torch::kByte &&
              packed.is_contiguous());
  const int K = (int)packed.size(1) * 2;
  const long N = packed.size(0);
  TORCH_CHECK(K % 8 == 0 && group % 8 == 0, "K/group alignment");
  auto out = torch::empty({N, K},
                          packed.options().dtype(torch::kBFloat16));
  launch_dequant_int4(packed.data_ptr(), scale.data_ptr<float>(),
                      out.data_ptr(), N, K, (int)group, cur_stream());
  return out;
}

// chunked-vocab CE: online LSE merge over one logits chunk (in-place
// m/l/tgt update) and the per-chunk dlogits for the dX sweep.
void xent_lse_merge(torch::Tensor logits, torch::Tensor targets,
                    torch::Tensor m_run, torch::Tensor l_run,
                    torch::Tensor tgt, long v0, long ignore_index) {
  check_bf16_contig(logits, "logits");
  const int Vc = (int)logits.size(-1);
  const long N = logits.numel() / Vc;
  TORCH_CHECK(Vc % 8 == 0, "Vc % 8");
  launch_xent_lse_merge(logits.data_ptr(), targets.data_ptr<long>(),
                        m_run.data_ptr<float>(), l_run.data_ptr<float>(),
                        tgt.data_ptr<float>(), N, Vc, v0, ignore_index,
                        cur_stream());
}

torch::Tensor xent_dlogits(torch::Tensor logits, torch::Tensor targets,
                           torch::Tensor lse, long v0, long ignore_index) {
  check_bf16_contig(logits, "logits");
  const int Vc = (int)logits.size(-1);
  const long N = logits.numel() / Vc;
  TORCH_CHECK(Vc % 8 == 0, "Vc % 8");
  auto dl = torch::empty_like(logits);
  launch_xent_dlogits(logits.data_ptr(), targets.data_ptr<long>(),
                      lse.data_ptr<float>(), dl.data_ptr(), N, Vc, v0,
                      ignore_index, cur_stream());
  return dl;
}

// y[1,N] = x[1,K] @ W[N,K]^T (decode GEMV; fp32 accumulate)
torch::Tensor gemv(torch::Tensor x, torch::Tensor w) {
  check_bf16_contig(x, "x");
  check_bf16_contig(w, "w");
  const int K = (int)w.size(1), N = (int)w.size(0);
  TORCH_CHECK(x.numel() == K, "gemv wants a single row");
  TORCH_CHECK(K % 8 == 0, "K % 8");
  auto sizes = x.sizes().vec();
  sizes[sizes.size() - 1] = N;
  auto y = torch::empty(sizes, x.options());
  launch_gemv_bf16(x.data_ptr(), w.data_ptr(), y.data_ptr(), N, K,
                   cur_stream());
  return y;
}

// Quantized decode: y[M,N] = x[M,K] @ dequant(Wq)[N,K]^T for M <= 16
// rows (the flattened leading dims of x), streaming the integer weight
// (qgemv.hip). Only allocation is the output: hipGraph-capturable.
static torch::Tensor qgemv_out(const torch::Tensor& x, int N) {
  auto sizes = x.sizes().vec();
  sizes[sizes.size() - 1] = N;
  return torch::empty(sizes, x.options());
}

static long qgemv_rows(const torch::Tensor& x, int K) {
  check_bf16_contig(x, "x");
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) == K, "qgemv: x inner dim != K");
  const long M = x.numel() / K;
  TORCH_CHECK(M >= 1 && M <= 16, "qgemv: 1 <= M <= 16, got ", M);
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0, "qgemv: x 16-B aligned");
  return M;
}

static void qgemv_check_w(const torch::Tensor& w, at::ScalarType dt,
                          const torch::Tensor& scale, long nscale) {
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == dt && w.dim() == 2 &&
              w.is_contiguous(), "qgemv: weight dtype/layout");
  TORCH_CHECK((uintptr_t)w.data_ptr() % 16 == 0,
              "qgemv: weight 16-B aligned");
  TORCH_CHECK(scale.is_cuda() && scale.scalar_type() == torch::kFloat &&
              scale.is_contiguous() && scale.numel() == nscale,
              "qgemv: scale dtype/shape");
}

torch::Tensor qgemv_int8(torch::Tensor x, torch::Tensor q,
                         torch::Tensor scale) {
  const int N = (int)q.size(0), K = (int)q.size(1);
  TORCH_CHECK(K > 0 && K % 16 == 0, "qgemv_int8: K % 16");
  qgemv_check_w(q, torch::kChar, scale, N);
  const long M = qgemv_rows(x, K);
  auto y = qgemv_out(x, N);
  launch_qgemv_int8(x.data_ptr(), q.data_ptr(), scale.data_ptr<float>(),
                    y.data_ptr(), (int)M, N, K, cur_stream());
  return y;
}

torch::Tensor qgemv_int4(torch::Tensor x, torch::Tensor packed,
                         torch::Tensor scale, long group) {
  const int N = (int)packed.size(0), K = (int)packed.size(1) * 2;
  TORCH_CHECK(K > 0 && K % 32 == 0, "qgemv_int4: K % 32");
  TORCH_CHECK(group > 0 && group % 32 == 0 && K % group == 0,
              "qgemv_int4: group % 32, K % group");
  qgemv_check_w(packed, torch::kByte, scale, (long)N * (K / group));
  const long M = qgemv_rows(x, K);
  auto y = qgemv_out(x, N);
  launch_qgemv_int4(x.data_ptr(), packed.data_ptr(),
                    scale.data_ptr<float>(), y.data_ptr(), (int)M, N, K,
                    (int)group, cur_stream());
  return y;
}

// Multi-adapter decode: y[m] += scale[g] * (x[m] @ A[g]^T) @ Bt[g] with
// g = idx[m] read ON THE DEVICE (mlora.hip); rows with an index outside
// [0,G) are left untouched. Nothing here looks at idx's content and the
// only allocation is t, so the call is hipGraph-capturable and a replay
// follows whatever idx holds by then.
void mlora_add(torch::Tensor y, torch::Tensor x, torch::Tensor A,
               torch::Tensor Bt, torch::Tensor scale, torch::Tensor idx) {
  check_bf16_contig(y, "y");
  check_bf16_contig(x, "x");
  check_bf16_contig(A, "A");
  check_bf16_contig(Bt, "Bt");
  TORCH_CHECK(y.dim() == 2 && x.dim() == 2 && A.dim() == 3 && Bt.dim() == 3,
              "mlora: y [M,N], x [M,K], A [G,R,K], Bt [G,R,N]");
  const long M = x.size(0), K = x.size(1), N = y.size(1);
  const long G = A.size(0), R = A.size(1);
  TORCH_CHECK(y.size(0) == M, "mlora: y/x rows differ");
  TORCH_CHECK(A.size(2) == K && Bt.size(0) == G && Bt.size(1) == R &&
              Bt.size(2) == N, "mlora: A [G,R,K] / Bt [G,R,N] mismatch");
  TORCH_CHECK(M >= 1 && M <= 16, "mlora: 1 <= M <= 16, got ", M);
  TORCH_CHECK(K >= 8 && K % 8 == 0 && N >= 8 && N % 8 == 0,
              "mlora: K % 8, N % 8");
  TORCH_CHECK(R == 8 || R == 16 || R == 32 || R == 64,
              "mlora: R must be 8, 16, 32 or 64, got ", R);
  TORCH_CHECK(G >= 1 && G * R * std::max(K, N) < (1L << 40),
              "mlora: stack size");
  TORCH_CHECK(scale.is_cuda() && scale.scalar_type() == torch::kFloat &&
              scale.is_contiguous() && scale.numel() == G,
              "mlora: scale must be f32 [G] on the GPU");
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == torch::kInt &&
              idx.is_contiguous() && idx.numel() == M,
              "mlora: idx must be int32 [M] on the GPU");
  TORCH_CHECK((uintptr_t)y.data_ptr() % 16 == 0 &&
              (uintptr_t)x.data_ptr() % 16 == 0 &&
              (uintptr_t)A.data_ptr() % 16 == 0 &&
              (uintptr_t)Bt.data_ptr() % 16 == 0, "mlora: 16-B alignment");
  auto t = torch::empty({M, R}, x.options().dtype(torch::kFloat));
  launch_mlora_shrink(x.data_ptr(), A.data_ptr(), idx.data_ptr<int>(),
                      t.data_ptr<float>(), (int)M, (int)K, (int)R, (int)G,
                      cur_stream());
  launch_mlora_expand_add(y.data_ptr(), t.data_ptr<float>(), Bt.data_ptr(),
                          scale.data_ptr<float>(), idx.data_ptr<int>(),
                          (int)M, (int)N, (int)R, (int)G, cur_stream());
}

// Per-row sampling of a decode batch (sample.hip): every parameter is a
// device tensor the kernel reads at run time and the only allocation is
// the output, so the call is hipGraph-capturable and a replay follows
// whatever the parameter buffers hold by then.
torch::Tensor sample(torch::Tensor logits, torch::Tensor temperature,
                     torch::Tensor top_p, torch::Tensor top_k,
                     torch::Tensor seed, torch::Tensor offset,
                     c10::optional<torch::Tensor> u) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == torch::kBFloat16,
              "sample: logits must be bf16 on the GPU");
  TORCH_CHECK(logits.dim() == 2, "sample: logits must be [B, V]");
  const long B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V > 0 && V % 8 == 0, "sample: V % 8, got V = ", V);
  TORCH_CHECK(V <= sample_max_vocab(), "sample: V = ", V,
              " is above the kernel limit of ", sample_max_vocab());
  TORCH_CHECK(logits.stride(1) == 1, "sample: logits rows must be dense");
  TORCH_CHECK(B <= 1 || (logits.stride(0) >= 0 && logits.stride(0) % 8 == 0),
              "sample: row stride % 8");
  TORCH_CHECK((uintptr_t)logits.data_ptr() % 16 == 0,
              "sample: logits need 16-B alignment");
  auto par = [&](const torch::Tensor& t, torch::ScalarType ty,
                 const char* name) {
    TORCH_CHECK(t.is_cuda() && t.get_device() == logits.get_device() &&
                t.scalar_type() == ty && t.dim() == 1 && t.size(0) == B &&
                t.is_contiguous(),
                "sample: ", name, " must be a contiguous ", ty, " [", B,
                "] tensor on the logits' device");
  };
  par(temperature, torch::kFloat, "temperature");
  par(top_p, torch::kFloat, "top_p");
  par(top_k, torch::kInt, "top_k");
  par(seed, torch::kLong, "seed");
  par(offset, torch::kInt, "offset");
  const float* up = nullptr;
  if (u.has_value()) {
    par(*u, torch::kFloat, "u");
    up = u->data_ptr<float>();
  }
  auto out = torch::empty({B}, logits.options().dtype(torch::kLong));
  if (B == 0) return out;
  launch_sample(logits.data_ptr(), B > 1 ? logits.stride(0) : V, (int)B,
                (int)V, temperature.data_ptr<float>(),
                top_p.data_ptr<float>(), top_k.data_ptr<int>(),
                (const long long*)seed.data_ptr<int64_t>(),
                offset.data_ptr<int>(), up,
                (long long*)out.data_ptr<int64_t>(), cur_stream());
  return out;
}

// Decode fast path: q [B,1,Hq,D] against the KV cache (flash-decoding
// split-KV partials; no V transpose needed).
std::vector<torch::Tensor> attn_decode(torch::Tensor q, torch::Tensor k,
                                       torch::Tensor v, double scale,
                                       c10::optional<torch::Tensor>
                                           len_dev) {
  check_bf16_contig(q, "q");
  const int B = (int)q.size(0), Hq = (int)q.size(2), D = (int)q.size(3);
  const int Skv = (int)k.size(1), Hkv = (int)k.size(2);
  // accept KV-cache VIEWS (prefix of a preallocated cache): inner
  // strides must be dense; the batch stride only matters for B > 1
  auto dense_kv = [&](const torch::Tensor& t, const char* n) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16,
                n, " must be bf16 GPU");
    TORCH_CHECK(t.stride(3) == 1 && t.stride(2) == D &&
                t.stride(1) == (long)Hkv * D,
                n, " must be s/h/d-dense");
    if (B > 1) TORCH_CHECK(t.is_contiguous(), n, " batch>1 needs contig");
  };
  dense_kv(k, "k");
  dense_kv(v, "v");
  TORCH_CHECK(q.size(1) == 1, "decode path wants S == 1");
  TORCH_CHECK(D == 64 || D == 128, "D must be 64 or 128");
  const int ns = attn_decode_nsplit(Skv);
  auto part = torch::empty({(long)B * Hq, ns, D + 2},
                           q.options().dtype(torch::kFloat));
  auto o = torch::empty_like(q);
  auto lse = torch::empty({B, Hq, 1}, q.options().dtype(torch::kFloat));
  const int* ld = nullptr;
  int len_stride = 0;
  if (len_dev.has_value()) {
    TORCH_CHECK(len_dev->scalar_type() == torch::kInt &&
                len_dev->is_cuda(), "len_dev must be int32 on GPU");
    ld = len_dev->data_ptr<int>();
    len_stride = len_dev->numel() > 1;
    if (len_stride)
      TORCH_CHECK(len_dev->numel() == B, "len_dev must be [1] or [B]");
  }
  launch_attn_decode(q.data_ptr(), k.data_ptr(), v.data_ptr(), ld,
                     part.data_ptr<float>(), o.data_ptr(),
                     lse.data_ptr<float>(), B, Hq, Hkv, Skv, D,
                     (float)scale, len_stride, cur_stream());
  return {o, lse};
}

// All BSHD, read in place: nothing is transposed on the host side.
std::vector<torch::Tensor> attn_bwd(torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, torch::Tensor o,
                                    torch::Tensor dO, torch::Tensor lse,
                                    bool causal, double scale,
                                    c10::optional<torch::Tensor> doc_start,
                                    c10::optional<torch::Tensor> doc_end) {
  check_bf16_contig(q, "q");
  check_bf16_contig(k, "k");
  check_bf16_contig(v, "v");
  auto dO_c = dO.contiguous();
  const int B = (int)q.size(0), S = (int)q.size(1), Hq = (int)q.size(2),
            D = (int)q.size(3);
  const int Skv = (int)k.size(1), Hkv = (int)k.size(2);
  check_bf16_contig(o, "o");
  const int* dsp = doc_map_ptr(doc_start, B, S, "doc_start");
  const int* dep = doc_map_ptr(doc_end, B, S, "doc_end");
  TORCH_CHECK((dsp == nullptr) == (dep == nullptr),
              "doc_start and doc_end go together");
  if (dsp) check_docs_shape(causal, S, Skv);
  auto delta = torch::empty({B, Hq, S}, q.options().dtype(torch::kFloat));
  // dkdv and dq gather their B-fragments from the ROW-major LDS tiles
  // with ds_read_b64_tr_b16 (tr_bfrag) — no pre-transposed Q/K/dO
  // copies, no transpose_sd pre-passes in the backward at all
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(v);
  // dq goes first: its prologue forms delta = rowsum(dO o O) from the dO
  // fragments it holds and writes it; dkdv, next on the same stream,
  // reads it. There is no separate delta pass.
  launch_attn_bwd_dq(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                     dO_c.data_ptr(), o.data_ptr(), lse.data_ptr<float>(),
                     delta.data_ptr<float>(), dq.data_ptr(), dsp, B, Hq,
                     Hkv, S, Skv, D, (float)scale, causal ? 1 : 0,
                     cur_stream());
  launch_attn_bwd_dkdv(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                       dO_c.data_ptr(), lse.data_ptr<float>(),
                       delta.data_ptr<float>(), dk.data_ptr(),
                       dv.data_ptr(), dep, B, Hq, Hkv, S, Skv, D,
                       (float)scale, causal ? 1 : 0, cur_stream());
  return {dq, dk, dv};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rmsnorm_fwd", &rmsnorm_fwd);
  m.def("rmsnorm_bwd", &rmsnorm_bwd, py::arg("dy"), py::arg("x"),
        py::arg("w"), py::arg("inv"), py::arg("dres") = py::none());
  m.def("rope", &rope, py::arg("x"), py::arg("cosb"), py::arg("sinb"),
        py::arg("pos0"), py::arg("backward"),
        py::arg("pos_dev") = py::none(),
        py::arg("doc_start") = py::none());
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("swiglu_bwd", &swiglu_bwd);
  m.def("xent_fwd", &xent_fwd);
  m.def("xent_bwd", &xent_bwd);
  m.def("xent_lse_merge", &xent_lse_merge);
  m.def("dequant_int8", &dequant_int8);
  m.def("dequant_int4", &dequant_int4);
  m.def("xent_dlogits", &xent_dlogits);
  m.def("lora_contract", &lora_contract, py::arg("x"), py::arg("w"),
        py::arg("mask") = py::none(), py::arg("seed") = 0,
        py::arg("keep") = 1.0);
  m.def("lora_wgrad", &lora_wgrad, py::arg("t"), py::arg("x"),
        py::arg("scale"), py::arg("mask") = py::none(),
        py::arg("seed") = 0, py::arg("keep") = 1.0);
  m.def("lora_contract2", &lora_contract2, py::arg("x"), py::arg("w0"),
        py::arg("w1"), py::arg("seed0") = 0, py::arg("seed1") = 0,
        py::arg("keep") = 1.0);
  m.def("lora_expand_add_t", &lora_expand_add_t, py::arg("y"),
        py::arg("t"), py::arg("wt"), py::arg("scale"),
        py::arg("mask") = py::none(), py::arg("seed") = 0,
        py::arg("keep") = 1.0);
  m.def("lora_expand_rng_ok", &lora_expand_rng_ok, py::arg("m"),
        py::arg("n"), py::arg("r"));
  m.def("lora_expand_add2", &lora_expand_add2, py::arg("y"), py::arg("t0"),
        py::arg("t1"), py::arg("a0"), py::arg("a1"), py::arg("scale"),
        py::arg("seed0") = 0, py::arg("seed1") = 0, py::arg("keep") = 1.0);
  m.def("dropout_mask", &dropout_mask, py::arg("m"), py::arg("k"),
        py::arg("seed"), py::arg("keep"), py::arg("like"));
  m.def("adamw", &adamw);
  m.def("l2_norm", &l2_norm);
  m.def("attn_fwd", &attn_fwd, py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("causal"), py::arg("scale"),
        py::arg("doc_start") = py::none());
  m.def("attn_bwd", &attn_bwd, py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("o"), py::arg("dO"), py::arg("lse"), py::arg("causal"),
        py::arg("scale"), py::arg("doc_start") = py::none(),
        py::arg("doc_end") = py::none());
  m.def("transpose_sd", &transpose_sd);
  m.def("gemv", &gemv);
  m.def("qgemv_int8", &qgemv_int8, py::arg("x"), py::arg("q"),
        py::arg("scale"));
  m.def("qgemv_int4", &qgemv_int4, py::arg("x"), py::arg("packed"),
        py::arg("scale"), py::arg("group") = 64);
  m.def("mlora_add", &mlora_add, py::arg("y"), py::arg("x"), py::arg("A"),
        py::arg("Bt"), py::arg("scale"), py::arg("idx"));
  m.def("sample", &sample, py::arg("logits"), py::arg("temperature"),
        py::arg("top_p"), py::arg("top_k"), py::arg("seed"),
        py::arg("offset"), py::arg("u") = py::none());
  m.def("sample_max_vocab", &sample_max_vocab);
  m.def("gemm_nt", &gemm_nt, py::arg("a"), py::arg("b"),
        py::arg("src") = py::none());
  m.def("attn_decode", &attn_decode, py::arg("q"), py::arg("k"),
        py::arg("v"), py::arg("scale"), py::arg("len_dev") = py::none());
}
