// Torch bindings for the gfx950 HIP kernel library. The kernels index their
// pointers unchecked, so these bindings are the single gate: every pointer
// a kernel dereferences is checked here for device, dtype, density and
// element count (docs/kernels.md, "Binding contract"); dtx_launch.h says
// what each launcher assumes. bf16 compute dtype, fp32 reductions.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>
#include <climits>

#include "dtx_launch.h"

namespace {

using torch::Tensor;
using OptTensor = c10::optional<torch::Tensor>;
constexpr auto BF16 = torch::kBFloat16;
constexpr auto F32 = torch::kFloat;
constexpr auto I32 = torch::kInt;
constexpr auto I64 = torch::kLong;

// A size on its way to an int parameter of a launcher.
static int i32(long v) {
  TORCH_CHECK(v >= INT_MIN && v <= INT_MAX, "size ", v, " exceeds int");
  return (int)v;
}

const char* dt_name(at::ScalarType ty) {
  switch (ty) {
    case at::kBFloat16: return "bf16";
    case at::kFloat: return "f32";
    case at::kInt: return "int32";
    case at::kLong: return "int64";
    case at::kChar: return "int8";
    default: return c10::toString(ty);
  }
}

// The check vocabulary. A binding opens with one Op over its first tensor
// and passes every other tensor through dev / dense / opt before it takes
// a data_ptr; these are the only places that look at a tensor's device,
// dtype and layout.
struct Op {
  const char* op;
  const Tensor& ref;
  hipStream_t stream;   // the current device's current stream

  // The first tensor pins the device: the launch goes to the CURRENT
  // device's stream; another GPU's tensor is refused, not followed. This
  // form checks the device alone (dropout_mask's `like`).
  Op(const char* op_, const Tensor& first, const char* name)
      : op(op_), ref(first) {
    TORCH_CHECK(first.is_cuda(), op, ": ", name, " must be on the GPU");
    const auto cur = at::cuda::getCurrentCUDAStream();
    stream = (hipStream_t)cur.stream();
    TORCH_CHECK(first.get_device() == cur.device_index(), op, ": ", name,
                " must be on the current GPU");
  }
  Op(const char* op_, const Tensor& first, at::ScalarType ty,
     const char* name, bool contiguous = true) : Op(op_, first, name) {
    contiguous ? dense(first, ty, name) : dev(first, ty, name);
  }
  // on the GPU of the first tensor, of dtype ty (any strides)
  const Tensor& dev(const Tensor& t, at::ScalarType ty,
                    const char* name) const {
    TORCH_CHECK(t.is_cuda() && t.get_device() == ref.get_device() &&
                t.scalar_type() == ty, op, ": ", name, " must be ",
                dt_name(ty), " on the GPU of the first argument");
    return t;
  }
  // dev + contiguous (+ exactly n elements)
  const Tensor& dense(const Tensor& t, at::ScalarType ty, const char* name,
                      long n = -1) const {
    TORCH_CHECK(dev(t, ty, name).is_contiguous(), op, ": ", name,
                " must be contiguous");
    TORCH_CHECK(n < 0 || t.numel() == n, op, ": ", name, " must be ", n,
                " elements long, got ", t.numel());
    return t;
  }
  void shape(const Tensor& t, at::IntArrayRef want, const char* name) const {
    TORCH_CHECK(t.sizes() == want, op, ": ", name, " must be ", want,
                ", got ", t.sizes());
  }
  // optional dense tensor: its pointer, or nullptr
  template <typename T = void>
  const T* opt(const OptTensor& t, at::ScalarType ty, const char* name,
               long n = -1) const {
    if (!t.has_value()) return nullptr;
    return static_cast<const T*>(dense(*t, ty, name, n).data_ptr());
  }
  // for the tensors a kernel reads or writes in 16-byte pieces
  void aligned16(const char* names,
                 std::initializer_list<const void*> ptrs) const {
    for (const void* p : ptrs)
      TORCH_CHECK((uintptr_t)p % 16 == 0, op, ": ", names,
                  " need 16-byte alignment");
  }
  // M of x [..., inner] (inner < 0: x's own last dimension, not empty)
  long rows(const Tensor& x, const char* name, long inner = -1) const {
    TORCH_CHECK(x.dim() >= 1 && x.size(-1) > 0, op, ": ", name,
                " must be [..., n] with n > 0");
    TORCH_CHECK(inner < 0 || x.size(-1) == inner, op, ": ", name,
                " must be [..., ", inner, "], got ", x.sizes());
    return x.numel() / x.size(-1);
  }
};

// Sequence-packing maps (doc_start / doc_end): int32 [B,S].
const int* doc_map(const Op& op, const OptTensor& t, long B, long S,
                   const char* name) {
  if (t.has_value()) op.shape(*t, {B, S}, name);
  return op.opt<int>(t, I32, name);
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

// x [M,H], w [H]: M
static long rmsnorm_rows(const Op& op, const Tensor& x, const Tensor& w) {
  const long M = op.rows(x, "x"), H = x.size(-1);
  TORCH_CHECK(H % 8 == 0, op.op, ": H % 8");
  TORCH_CHECK(H <= RMSNORM_MAX_H, "rmsnorm: H = ", H,
              " is above the kernel limit of ", RMSNORM_MAX_H);
  op.dense(w, BF16, "w", H);
  op.aligned16("x, w", {x.data_ptr(), w.data_ptr()});
  return M;
}

std::vector<Tensor> rmsnorm_fwd(Tensor x, Tensor w, double eps) {
  const Op op("rmsnorm_fwd", x, BF16, "x");
  const int M = i32(rmsnorm_rows(op, x, w)), H = i32(x.size(-1));
  auto y = torch::empty_like(x);
  auto inv = torch::empty({M}, x.options().dtype(F32));
  if (M == 0) return {y, inv};
  launch_rmsnorm_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(),
                     inv.data_ptr<float>(), M, H, (float)eps, op.stream);
  return {y, inv};
}

std::vector<Tensor> rmsnorm_bwd(Tensor dy, Tensor x, Tensor w, Tensor inv,
                                OptTensor dres) {
  const Op op("rmsnorm_bwd", dy, BF16, "dy");
  op.dense(x, BF16, "x");
  const int M = i32(rmsnorm_rows(op, x, w)), H = i32(x.size(-1));
  op.shape(dy, x.sizes(), "dy");
  op.dense(inv, F32, "inv", M);
  const void* drp = op.opt(dres, BF16, "dres", x.numel());
  op.aligned16("dy, dres", {dy.data_ptr(), drp});
  auto dx = torch::empty_like(x);
  if (M == 0) return {dx, torch::zeros({H}, x.options().dtype(F32))};
  auto dw = torch::empty({H}, x.options().dtype(F32));
  auto part = torch::empty({rmsnorm_bwd_nblocks(M), H}, dw.options());
  launch_rmsnorm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(),
                     inv.data_ptr<float>(), drp, dx.data_ptr(),
                     part.data_ptr<float>(), dw.data_ptr<float>(), M, H,
                     op.stream);
  return {dx, dw};
}

// ---------------------------------------------------------------- RoPE
// The values inside pos_dev are the caller's contract (dtx_launch.h).
Tensor rope(Tensor x, Tensor cosb, Tensor sinb, long pos0, bool backward,
            OptTensor pos_dev, OptTensor doc_start) {
  const Op op("rope", x, BF16, "x");
  TORCH_CHECK(x.dim() == 4, "rope: x must be [B,S,H,D]");
  const long B = x.size(0);
  const int S = i32(x.size(1)), H = i32(x.size(2)), D = i32(x.size(3));
  TORCH_CHECK(D % 8 == 0, "rope: D % 8");
  TORCH_CHECK(pos0 >= 0, "rope: pos0 must be >= 0");
  op.dense(cosb, F32, "cosb");
  TORCH_CHECK(cosb.dim() == 2 && cosb.size(1) == D / 2,
              "rope: cosb must be [rows, D/2]");
  op.shape(op.dense(sinb, F32, "sinb"), cosb.sizes(), "sinb");
  op.aligned16("cosb, sinb", {cosb.data_ptr(), sinb.data_ptr()});
  const int* dsp = doc_map(op, doc_start, B, S, "doc_start");
  TORCH_CHECK(!(dsp && pos_dev.has_value()),
              "doc_start cannot be combined with pos_dev");
  const int* pd = op.opt<int>(pos_dev, I32, "pos_dev");
  TORCH_CHECK(!pd || pos_dev->numel() == 1 || pos_dev->numel() == B,
              "rope: pos_dev must be [1] or [B]");
  const int pos_per_b = pd && pos_dev->numel() > 1;
  TORCH_CHECK(cosb.size(0) >= (pd ? S : pos0 + S), "rope table too short");
  auto y = torch::empty_like(x);
  if (x.numel() == 0) return y;
  launch_rope(x.data_ptr(), cosb.data_ptr<float>(), sinb.data_ptr<float>(),
              y.data_ptr(), B, S, H, D, i32(pos0), backward ? 1 : 0, pd,
              pos_per_b, dsp, op.stream);
  return y;
}

// --------------------------------------------------------------- SwiGLU
Tensor swiglu_fwd(Tensor gate, Tensor up) {
  const Op op("swiglu_fwd", gate, BF16, "gate");
  op.shape(op.dense(up, BF16, "up"), gate.sizes(), "up");
  TORCH_CHECK(gate.numel() % 8 == 0, "swiglu_fwd: numel % 8");
  op.aligned16("gate, up", {gate.data_ptr(), up.data_ptr()});
  auto out = torch::empty_like(gate);
  if (gate.numel() == 0) return out;
  launch_swiglu_fwd(gate.data_ptr(), up.data_ptr(), out.data_ptr(),
                    gate.numel(), op.stream);
  return out;
}

std::vector<Tensor> swiglu_bwd(Tensor dout, Tensor gate, Tensor up) {
  const Op op("swiglu_bwd", dout, BF16, "dout");
  op.shape(op.dense(gate, BF16, "gate"), dout.sizes(), "gate");
  op.shape(op.dense(up, BF16, "up"), dout.sizes(), "up");
  TORCH_CHECK(gate.numel() % 8 == 0, "swiglu_bwd: numel % 8");
  op.aligned16("dout, gate, up",
               {dout.data_ptr(), gate.data_ptr(), up.data_ptr()});
  auto dg = torch::empty_like(gate);
  auto du = torch::empty_like(up);
  if (gate.numel() == 0) return {dg, du};
  launch_swiglu_bwd(dout.data_ptr(), gate.data_ptr(), up.data_ptr(),
                    dg.data_ptr(), du.data_ptr(), gate.numel(),
                    op.stream);
  return {dg, du};
}

// -------------------------------------------------------- cross entropy
// logits [N,V] in whole 16-byte groups, targets [N] int64: N. Target
// VALUES are not inspected (that would be a host sync): caller's contract.
static long xent_rows(const Op& op, const Tensor& logits, const Tensor& tg) {
  const long N = op.rows(logits, "logits");
  TORCH_CHECK(logits.size(-1) % 8 == 0, op.op, ": V % 8");
  op.aligned16("logits", {logits.data_ptr()});
  op.dense(tg, I64, "targets", N);
  return N;
}

std::vector<Tensor> xent_fwd(Tensor logits, Tensor targets, long ignore) {
  const Op op("xent_fwd", logits, BF16, "logits");
  const long N = xent_rows(op, logits, targets);
  const int V = i32(logits.size(-1));
  auto loss = torch::empty({N}, logits.options().dtype(F32));
  auto lse = torch::empty_like(loss);
  if (N == 0) return {loss, lse};
  launch_xent_fwd(logits.data_ptr(), targets.data_ptr<long>(),
                  loss.data_ptr<float>(), lse.data_ptr<float>(), N, V,
                  ignore, op.stream);
  return {loss, lse};
}

Tensor xent_bwd(Tensor logits, Tensor targets, Tensor lse, Tensor dloss,
                long ignore) {
  const Op op("xent_bwd", logits, BF16, "logits");
  const long N = xent_rows(op, logits, targets);
  const int V = i32(logits.size(-1));
  op.dense(lse, F32, "lse", N);
  op.dense(dloss, F32, "dloss", N);
  auto dlogits = torch::empty_like(logits);
  if (N == 0) return dlogits;
  launch_xent_bwd(logits.data_ptr(), targets.data_ptr<long>(),
                  lse.data_ptr<float>(), dloss.data_ptr<float>(),
                  dlogits.data_ptr(), N, V, ignore, op.stream);
  return dlogits;
}

// chunked-vocab CE: online LSE merge over one logits chunk (in-place
// m/l/tgt update) and the per-chunk dlogits for the dX sweep.
void xent_lse_merge(Tensor logits, Tensor targets, Tensor m_run,
                    Tensor l_run, Tensor tgt, long v0, long ignore_index) {
  const Op op("xent_lse_merge", logits, BF16, "logits");
  const long N = xent_rows(op, logits, targets);
  const int Vc = i32(logits.size(-1));
  TORCH_CHECK(v0 >= 0, "xent_lse_merge: v0 must be >= 0");
  op.dense(m_run, F32, "m_run", N);
  op.dense(l_run, F32, "l_run", N);
  op.dense(tgt, F32, "tgt", N);
  if (N == 0) return;
  launch_xent_lse_merge(logits.data_ptr(), targets.data_ptr<long>(),
                        m_run.data_ptr<float>(), l_run.data_ptr<float>(),
                        tgt.data_ptr<float>(), N, Vc, v0, ignore_index,
                        op.stream);
}

Tensor xent_dlogits(Tensor logits, Tensor targets, Tensor lse, long v0,
                    long ignore_index) {
  const Op op("xent_dlogits", logits, BF16, "logits");
  const long N = xent_rows(op, logits, targets);
  const int Vc = i32(logits.size(-1));
  TORCH_CHECK(v0 >= 0, "xent_dlogits: v0 must be >= 0");
  op.dense(lse, F32, "lse", N);
  auto dl = torch::empty_like(logits);
  if (N == 0) return dl;
  launch_xent_dlogits(logits.data_ptr(), targets.data_ptr<long>(),
                      lse.data_ptr<float>(), dl.data_ptr(), N, Vc, v0,
                      ignore_index, op.stream);
  return dl;
}

// ----------------------------------------------------------------- LoRA
// Dropout enters as an optional `mask` (bf16, same shape as x / y; no
// mask-multiply materialization) or as seed + keep < 1 (in-kernel RNG).
// The kernels read the rows of x, y and of the adapters [r, inner] in
// 16-byte pieces: inner % 8, aligned bases.

// x or y [M, inner]: M
static long lora_rows(const Op& op, const Tensor& x, const char* name) {
  const long M = op.rows(x, name);
  TORCH_CHECK(x.size(-1) % 8 == 0, op.op, ": ", name, " width % 8");
  op.aligned16(name, {x.data_ptr()});
  return M;
}

// adapter [r, inner] with r >= 1, and r <= rmax where rmax > 0: r
static int lora_rank(const Op& op, const Tensor& w, const char* name,
                     long inner, long rmax = 0) {
  op.dense(w, BF16, name);
  TORCH_CHECK(w.dim() == 2 && w.size(1) == inner && w.size(0) >= 1, op.op,
              ": ", name, " must be [r,", inner, "] with r >= 1, got ",
              w.sizes());
  TORCH_CHECK(rmax <= 0 || w.size(0) <= rmax, op.op, ": r <= ", rmax,
              ", got ", name, " ", w.sizes());
  op.aligned16(name, {w.data_ptr()});
  return i32(w.size(0));
}

void check_keep(const Op& op, double keep) {
  TORCH_CHECK(keep > 0.0 && keep <= 1.0, op.op, ": 0 < keep <= 1");
}

// fp32 split-K planes of the contract kernels (none when one slice does)
float* contract_part(Tensor& part, const Tensor& t, int K, long M, int r) {
  const int nsplit = lora_contract_ksplit(K, M, r);
  if (nsplit <= 1) return nullptr;
  part = torch::empty({nsplit, t.numel()}, t.options());
  return part.data_ptr<float>();
}

Tensor lora_contract(Tensor x, Tensor w, OptTensor mask, int64_t seed,
                     double keep) {
  const Op op("lora_contract", x, BF16, "x");
  const long M = lora_rows(op, x, "x");
  const int K = i32(x.size(-1)), r = lora_rank(op, w, "w", K, 64);
  check_keep(op, keep);
  const void* mk = op.opt(mask, BF16, "mask", x.numel());
  op.aligned16("mask", {mk});
  auto t = torch::empty({M, r}, x.options().dtype(F32));
  if (M == 0) return t;
  Tensor part;
  float* part_ptr = contract_part(part, t, K, M, r);
  launch_lora_contract(x.data_ptr(), w.data_ptr(), mk, part_ptr,
                       t.data_ptr<float>(), M, K, r,
                       (unsigned long long)seed, (float)keep, op.stream);
  return t;
}

// Two adapters, two dropout seeds, one pass over x: (t0, t1), each
// bit-identical to lora_contract with its own adapter and seed.
std::vector<Tensor> lora_contract2(Tensor x, Tensor w0, Tensor w1,
                                   int64_t seed0, int64_t seed1,
                                   double keep) {
  const Op op("lora_contract2", x, BF16, "x");
  const long M = lora_rows(op, x, "x");
  const int K = i32(x.size(-1)), r = lora_rank(op, w0, "w0", K, 16);
  op.shape(w1, w0.sizes(), "w1");
  lora_rank(op, w1, "w1", K, 16);
  check_keep(op, keep);
  auto t = torch::empty({2, M, r}, x.options().dtype(F32));
  if (M == 0) return {t[0], t[1]};
  Tensor part;
  float* part_ptr = contract_part(part, t, K, M, r);
  launch_lora_contract2(x.data_ptr(), w0.data_ptr(), w1.data_ptr(),
                        part_ptr, t.data_ptr<float>(), M, K, r,
                        (unsigned long long)seed0,
                        (unsigned long long)seed1, (float)keep,
                        op.stream);
  return {t[0], t[1]};
}

// wt is the adapter already in [r,N] (lora_B transposed, or lora_A as it
// is for the dx term): no transposed copy per call.
void lora_expand_add_t(Tensor y, Tensor t, Tensor wt, double scale,
                       OptTensor mask, int64_t seed, double keep) {
  const Op op("lora_expand_add_t", y, BF16, "y");
  const long M = lora_rows(op, y, "y");
  const int N = i32(y.size(-1)), r = lora_rank(op, wt, "wt", N);
  check_keep(op, keep);
  op.dense(t, F32, "t", M * r);
  const void* mk = op.opt(mask, BF16, "mask", y.numel());
  op.aligned16("mask", {mk});
  TORCH_CHECK(keep >= 1.0 || lora_expand_rng_ok(M, N, r),
              "RNG dropout needs the r<=16 fast path; materialize the "
              "mask for this shape");
  if (M == 0) return;
  launch_lora_expand_add(y.data_ptr(), t.data_ptr<float>(), wt.data_ptr(),
                         mk, M, N, r, (float)scale,
                         (unsigned long long)seed, (float)keep,
                         op.stream);
}

// y += mask0 o (s * t0 @ a0) + mask1 o (s * t1 @ a1), a0/a1 [r,N]: one
// read-modify-write of y, one rounding.
void lora_expand_add2(Tensor y, Tensor t0, Tensor t1, Tensor a0, Tensor a1,
                      double scale, int64_t seed0, int64_t seed1,
                      double keep) {
  const Op op("lora_expand_add2", y, BF16, "y");
  const long M = lora_rows(op, y, "y");
  const int N = i32(y.size(-1)), r = lora_rank(op, a0, "a0", N, 16);
  op.shape(a1, a0.sizes(), "a1");
  lora_rank(op, a1, "a1", N, 16);
  check_keep(op, keep);
  op.dense(t0, F32, "t0", M * r);
  op.dense(t1, F32, "t1", M * r);
  if (M == 0) return;
  launch_lora_expand_add_dual(y.data_ptr(), t0.data_ptr<float>(),
                              t1.data_ptr<float>(), a0.data_ptr(),
                              a1.data_ptr(), M, N, r, (float)scale,
                              (unsigned long long)seed0,
                              (unsigned long long)seed1, (float)keep,
                              op.stream);
}

Tensor lora_wgrad(Tensor t, Tensor x, double scale, OptTensor mask,
                  int64_t seed, double keep) {
  const Op op("lora_wgrad", x, BF16, "x");
  const long M = lora_rows(op, x, "x");
  const int K = i32(x.size(-1));
  const int r = op.dense(t, F32, "t").dim() >= 1 ? i32(t.size(-1)) : 0;
  TORCH_CHECK(r >= 1 && t.numel() == M * r, "lora_wgrad: t must be [M,r] ",
              "with M = ", M, ", r >= 1, got ", t.sizes());
  check_keep(op, keep);
  const void* mk = op.opt(mask, BF16, "mask", x.numel());
  op.aligned16("mask", {mk});
  if (M == 0) return torch::zeros({r, K}, x.options().dtype(F32));
  auto out = torch::empty({r, K}, x.options().dtype(F32));
  auto part = torch::empty({lora_wgrad_splitm(K, r, M), r, K},
                           out.options());
  launch_lora_wgrad(t.data_ptr<float>(), x.data_ptr(), mk,
                    part.data_ptr<float>(), out.data_ptr<float>(), M, K, r,
                    (float)scale, (unsigned long long)seed, (float)keep,
                    op.stream);
  return out;
}

// Materialize the RNG dropout mask (bit-identical to what the fused MODE==2
// kernels consume): tests and the r>16 fallback. `like` names the device.
Tensor dropout_mask(int64_t M, int64_t K, int64_t seed, double keep,
                    Tensor like) {
  const Op op("dropout_mask", like, "like");
  TORCH_CHECK(M >= 0 && K >= 0 && (M * K) % 8 == 0,
              "dropout_mask: M*K % 8 == 0");
  check_keep(op, keep);
  auto m = torch::empty({M, K}, like.options().dtype(BF16));
  if (M * K == 0) return m;
  launch_dropout_mask(m.data_ptr(), M * K, (unsigned long long)seed,
                      (float)keep, op.stream);
  return m;
}

// ---------------------------------------------------------------- AdamW
void adamw(Tensor p, Tensor master, Tensor grad, Tensor m, Tensor v,
           double lr, double b1, double b2, double eps, double wd,
           long step) {
  const Op op("adamw", p, BF16, "p");
  const long n = p.numel();
  TORCH_CHECK(n % 4 == 0, "flat param buffer must be padded to 4");
  TORCH_CHECK(step >= 1 && step <= INT_MAX, "adamw: step must be >= 1");
  op.dense(master, F32, "master", n);
  op.dense(grad, F32, "grad", n);
  op.dense(m, F32, "m", n);
  op.dense(v, F32, "v", n);
  op.aligned16("master, grad, m, v", {master.data_ptr(), grad.data_ptr(),
                                      m.data_ptr(), v.data_ptr()});
  if (n == 0) return;
  launch_adamw(p.data_ptr(), master.data_ptr<float>(),
               grad.data_ptr<float>(), m.data_ptr<float>(),
               v.data_ptr<float>(), n, (float)lr, (float)b1, (float)b2,
               (float)eps, (float)wd, (int)step, op.stream);
}

Tensor l2_norm(Tensor x) {
  const Op op("l2_norm", x, F32, "x");
  auto ws = torch::empty({1024}, x.options());
  auto out = torch::empty({1}, x.options());
  launch_l2_norm(x.data_ptr<float>(), ws.data_ptr<float>(),
                 out.data_ptr<float>(), x.numel(), op.stream);
  return out;
}

// ------------------------------------------------------------ attention
// [B,S,H,D] -> [B,H,D,S]
Tensor transpose_sd(Tensor x) {
  const Op op("transpose_sd", x, BF16, "x");
  TORCH_CHECK(x.dim() == 4, "transpose_sd: x must be [B,S,H,D]");
  const int B = i32(x.size(0)), S = i32(x.size(1)), H = i32(x.size(2)),
            D = i32(x.size(3));
  TORCH_CHECK(D % 64 == 0, "transpose_sd: D % 64");
  op.aligned16("x", {x.data_ptr()});
  auto xt = torch::empty({B, H, D, S}, x.options());
  if (x.numel() == 0) return xt;
  launch_transpose_sd(x.data_ptr(), xt.data_ptr(), B, S, H, D,
                      op.stream);
  return xt;
}

// q [B,S,Hq,D] (the Op's first tensor); k, v [B,Skv,Hkv,D] — all BSHD, v
// row-major like k. The launchers run nothing for another D.
struct AttnShape { int B, S, Hq, D, Skv, Hkv; };

AttnShape check_attn(const Op& op, const Tensor& q, const Tensor& k,
                     const Tensor& v) {
  TORCH_CHECK(q.dim() == 4, op.op, ": q must be [B,S,Hq,D]");
  const long B = q.size(0), D = q.size(3);
  TORCH_CHECK(D == 64 || D == 128, op.op, ": D must be 64 or 128");
  op.dense(k, BF16, "k");
  TORCH_CHECK(k.dim() == 4 && k.size(0) == B && k.size(3) == D, op.op,
              ": k must be [B,Skv,Hkv,D], got ", k.sizes());
  op.shape(op.dense(v, BF16, "v"), k.sizes(), "v");
  const AttnShape a{i32(B), i32(q.size(1)), i32(q.size(2)),
                    i32(D), i32(k.size(1)), i32(k.size(2))};
  TORCH_CHECK(a.S >= 1 && a.Skv >= 1, op.op, ": S >= 1 and Skv >= 1");
  TORCH_CHECK(a.Hkv >= 1 && a.Hq >= 1 && a.Hq % a.Hkv == 0, op.op,
              ": Hq % Hkv (GQA group)");
  op.aligned16("q, k, v", {q.data_ptr(), k.data_ptr(), v.data_ptr()});
  return a;
}

std::vector<Tensor> attn_fwd(Tensor q, Tensor k, Tensor v, bool causal,
                             double scale, OptTensor doc_start) {
  const Op op("attn_fwd", q, BF16, "q");
  const AttnShape a = check_attn(op, q, k, v);
  const int* dsp = doc_map(op, doc_start, a.B, a.S, "doc_start");
  if (dsp) check_docs_shape(causal, a.S, a.Skv);
  auto o = torch::empty_like(q);
  auto lse = torch::empty({a.B, a.Hq, a.S}, q.options().dtype(F32));
  if (a.B == 0) return {o, lse};
  launch_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                  lse.data_ptr<float>(), dsp, a.B, a.Hq, a.Hkv, a.S, a.Skv,
                  a.D, (float)scale, causal ? 1 : 0, op.stream);
  return {o, lse};
}

// C[M,N] = A[M,K] @ B[N,K]^T (+ optional bf16 src) — the hand-written
// 256x256-tile MFMA GEMM (gemm.hip). Requires N % 256 == 0, K % 64 == 0,
// K >= 128; any M (SRSRC-clamped tail).
Tensor gemm_nt(Tensor a, Tensor b, OptTensor src) {
  const Op op("gemm_nt", a, BF16, "a");
  TORCH_CHECK(op.dense(b, BF16, "b").dim() == 2, "gemm_nt: b must be [N,K]");
  const int K = i32(b.size(1)), N = i32(b.size(0));
  TORCH_CHECK(N % 256 == 0 && K % 64 == 0 && K >= 128,
              "gemm_nt: unsupported shape N=", N, " K=", K);
  const long M = op.rows(a, "a", K);
  const void* sp = op.opt(src, BF16, "src", M * (long)N);
  op.aligned16("a, b, src", {a.data_ptr(), b.data_ptr(), sp});
  auto sizes = a.sizes().vec();
  sizes.back() = N;
  auto c = torch::empty(sizes, a.options());
  if (M == 0 || N == 0) return c;
  launch_gemm_nt(a.data_ptr(), b.data_ptr(), sp, c.data_ptr(), M, N, K,
                 op.stream);
  return c;
}

// weight-only dequant (int8 per-row / int4 group-wise) -> bf16
Tensor dequant_int8(Tensor q, Tensor scale) {
  const Op op("dequant_int8", q, torch::kChar, "q");
  TORCH_CHECK(q.dim() == 2, "dequant_int8: q must be [N,K]");
  const long N = q.size(0);
  const int K = i32(q.size(1));
  TORCH_CHECK(K % 8 == 0, "dequant_int8: K % 8");
  op.dense(scale, F32, "scale", N);
  auto out = torch::empty({N, K}, q.options().dtype(BF16));
  if (q.numel() == 0) return out;
  launch_dequant_int8(q.data_ptr(), scale.data_ptr<float>(),
                      out.data_ptr(), N, K, op.stream);
  return out;
}

Tensor dequant_int4(Tensor packed, Tensor scale, long group) {
  const Op op("dequant_int4", packed, torch::kByte, "packed");
  TORCH_CHECK(packed.dim() == 2, "dequant_int4: packed must be [N,K/2]");
  const long N = packed.size(0);
  const int K = i32(packed.size(1) * 2);
  TORCH_CHECK(K % 8 == 0 && group > 0 && group % 8 == 0 && K % group == 0,
              "dequant_int4: K % 8, group % 8, K % group");
  op.dense(scale, F32, "scale", N * (K / group));
  auto out = torch::empty({N, K}, packed.options().dtype(BF16));
  if (packed.numel() == 0) return out;
  launch_dequant_int4(packed.data_ptr(), scale.data_ptr<float>(),
                      out.data_ptr(), N, K, i32(group), op.stream);
  return out;
}

// y[..., N] = x[..., K] @ W[N,K]^T, one row x (decode GEMV; fp32 accumulate)
Tensor gemv(Tensor x, Tensor w) {
  const Op op("gemv", x, BF16, "x");
  TORCH_CHECK(op.dense(w, BF16, "w").dim() == 2, "gemv: w must be [N,K]");
  const int K = i32(w.size(1)), N = i32(w.size(0));
  TORCH_CHECK(K % 8 == 0, "gemv: K % 8");
  TORCH_CHECK(op.rows(x, "x", K) == 1, "gemv wants a single row");
  op.aligned16("x, w", {x.data_ptr(), w.data_ptr()});
  auto sizes = x.sizes().vec();
  sizes.back() = N;
  auto y = torch::empty(sizes, x.options());
  if (N == 0) return y;
  launch_gemv_bf16(x.data_ptr(), w.data_ptr(), y.data_ptr(), N, K,
                   op.stream);
  return y;
}

// Quantized decode: y[M,N] = x[M,K] @ dequant(Wq)[N,K]^T for M <= 16
// rows (the flattened leading dims of x), streaming the integer weight
// (qgemv.hip). Only allocation is the output: hipGraph-capturable.
// Checks x [M,K] against the weight [N, cols] and its `nscale` scales,
// allocates y.
Tensor qgemv_out(const Op& op, const Tensor& x, const Tensor& w,
                 at::ScalarType wt, const Tensor& scale, int K,
                 long nscale) {
  op.dense(w, wt, "weight");
  op.dense(scale, F32, "scale", nscale);
  const long M = op.rows(x, "x", K);
  TORCH_CHECK(M >= 1 && M <= 16, "qgemv: 1 <= M <= 16, got ", M);
  op.aligned16("x, weight", {x.data_ptr(), w.data_ptr()});
  auto sizes = x.sizes().vec();
  sizes.back() = w.size(0);
  return torch::empty(sizes, x.options());
}

Tensor qgemv_int8(Tensor x, Tensor q, Tensor scale) {
  const Op op("qgemv_int8", x, BF16, "x");
  TORCH_CHECK(q.dim() == 2, "qgemv_int8: q must be [N,K]");
  const int N = i32(q.size(0)), K = i32(q.size(1));
  TORCH_CHECK(K > 0 && K % 16 == 0, "qgemv_int8: K % 16");
  auto y = qgemv_out(op, x, q, torch::kChar, scale, K, N);
  if (N == 0) return y;
  launch_qgemv_int8(x.data_ptr(), q.data_ptr(), scale.data_ptr<float>(),
                    y.data_ptr(), i32(x.numel() / K), N, K, op.stream);
  return y;
}

Tensor qgemv_int4(Tensor x, Tensor packed, Tensor scale, long group) {
  const Op op("qgemv_int4", x, BF16, "x");
  TORCH_CHECK(packed.dim() == 2, "qgemv_int4: packed must be [N,K/2]");
  const int N = i32(packed.size(0)), K = i32(packed.size(1) * 2);
  TORCH_CHECK(K > 0 && K % 32 == 0, "qgemv_int4: K % 32");
  TORCH_CHECK(group > 0 && group % 32 == 0 && K % group == 0,
              "qgemv_int4: group % 32, K % group");
  auto y = qgemv_out(op, x, packed, torch::kByte, scale, K,
                     (long)N * (K / group));
  if (N == 0) return y;
  launch_qgemv_int4(x.data_ptr(), packed.data_ptr(),
                    scale.data_ptr<float>(), y.data_ptr(), i32(x.numel() / K),
                    N, K, i32(group), op.stream);
  return y;
}

// Multi-adapter decode: y[m] += scale[g] * (x[m] @ A[g]^T) @ Bt[g] with
// g = idx[m] read ON THE DEVICE (mlora.hip); rows with an index outside
// [0,G) are left untouched. Nothing here looks at idx's content and the
// only allocation is t, so the call is hipGraph-capturable and a replay
// follows whatever idx holds by then.
void mlora_add(Tensor y, Tensor x, Tensor A, Tensor Bt, Tensor scale,
               Tensor idx) {
  const Op op("mlora", y, BF16, "y");
  op.dense(x, BF16, "x");
  op.dense(A, BF16, "A");
  op.dense(Bt, BF16, "Bt");
  TORCH_CHECK(y.dim() == 2 && x.dim() == 2 && A.dim() == 3 && Bt.dim() == 3,
              "mlora: y [M,N], x [M,K], A [G,R,K], Bt [G,R,N]");
  const int M = i32(x.size(0)), K = i32(x.size(1)), N = i32(y.size(1));
  const int G = i32(A.size(0)), R = i32(A.size(1));
  TORCH_CHECK(y.size(0) == M, "mlora: y/x rows differ");
  TORCH_CHECK(A.size(2) == K, "mlora: A [G,R,K] / Bt [G,R,N] mismatch");
  op.shape(Bt, {G, R, N}, "Bt");
  TORCH_CHECK(M >= 1 && M <= 16, "mlora: 1 <= M <= 16, got ", M);
  TORCH_CHECK(K >= 8 && K % 8 == 0 && N >= 8 && N % 8 == 0,
              "mlora: K % 8, N % 8");
  TORCH_CHECK(R == 8 || R == 16 || R == 32 || R == 64,
              "mlora: R must be 8, 16, 32 or 64, got ", R);
  TORCH_CHECK(G >= 1 && (long)G * R * std::max(K, N) < (1L << 40),
              "mlora: stack size");
  op.dense(scale, F32, "scale", G);
  op.dense(idx, I32, "idx", M);
  op.aligned16("y, x, A, Bt", {y.data_ptr(), x.data_ptr(), A.data_ptr(),
                               Bt.data_ptr()});
  auto t = torch::empty({M, R}, x.options().dtype(F32));
  launch_mlora_shrink(x.data_ptr(), A.data_ptr(), idx.data_ptr<int>(),
                      t.data_ptr<float>(), M, K, R, G, op.stream);
  launch_mlora_expand_add(y.data_ptr(), t.data_ptr<float>(), Bt.data_ptr(),
                          scale.data_ptr<float>(), idx.data_ptr<int>(), M,
                          N, R, G, op.stream);
}

// Per-row sampling of a decode batch (sample.hip): every parameter is a
// device tensor the kernel reads at run time and the only allocation is
// the output, so the call is hipGraph-capturable and a replay follows
// whatever the parameter buffers hold by then.
Tensor sample(Tensor logits, Tensor temperature, Tensor top_p, Tensor top_k,
              Tensor seed, Tensor offset, OptTensor u) {
  const Op op("sample", logits, BF16, "logits", /*contiguous=*/false);
  TORCH_CHECK(logits.dim() == 2, "sample: logits must be [B, V]");
  const int B = i32(logits.size(0)), V = i32(logits.size(1));
  TORCH_CHECK(V > 0 && V % 8 == 0, "sample: V % 8, got V = ", V);
  TORCH_CHECK(V <= sample_max_vocab(), "sample: V = ", V,
              " is above the kernel limit of ", sample_max_vocab());
  TORCH_CHECK(logits.stride(1) == 1, "sample: logits rows must be dense");
  TORCH_CHECK(B <= 1 || (logits.stride(0) >= 0 && logits.stride(0) % 8 == 0),
              "sample: row stride % 8");
  op.aligned16("logits", {logits.data_ptr()});
  op.shape(op.dense(temperature, F32, "temperature"), {B}, "temperature");
  op.shape(op.dense(top_p, F32, "top_p"), {B}, "top_p");
  op.shape(op.dense(top_k, I32, "top_k"), {B}, "top_k");
  op.shape(op.dense(seed, I64, "seed"), {B}, "seed");
  op.shape(op.dense(offset, I32, "offset"), {B}, "offset");
  if (u.has_value()) op.shape(*u, {B}, "u");
  const float* up = op.opt<float>(u, F32, "u");
  auto out = torch::empty({B}, logits.options().dtype(I64));
  if (B == 0) return out;
  launch_sample(logits.data_ptr(), B > 1 ? logits.stride(0) : (long)V, B, V,
                temperature.data_ptr<float>(), top_p.data_ptr<float>(),
                top_k.data_ptr<int>(),
                (const long long*)seed.data_ptr<int64_t>(),
                offset.data_ptr<int>(), up,
                (long long*)out.data_ptr<int64_t>(), op.stream);
  return out;
}

// Decode fast path: q [B,1,Hq,D] against the KV cache (flash-decoding
// split-KV partials; no V transpose needed). k and v may be VIEWS (the
// prefix of a preallocated cache): the inner strides must be dense, the
// batch stride only matters for B > 1. The values inside len_dev (<= Skv)
// are the caller's contract.
std::vector<Tensor> attn_decode(Tensor q, Tensor k, Tensor v, double scale,
                                OptTensor len_dev) {
  const Op op("attn_decode", q, BF16, "q");
  TORCH_CHECK(q.dim() == 4 && q.size(1) == 1,
              "attn_decode: q must be [B,1,Hq,D] (decode path wants S == 1)");
  const int B = i32(q.size(0)), Hq = i32(q.size(2)), D = i32(q.size(3));
  TORCH_CHECK(D == 64 || D == 128, "attn_decode: D must be 64 or 128");
  TORCH_CHECK(op.dev(k, BF16, "k").dim() == 4 && k.size(0) == B &&
              k.size(3) == D, "attn_decode: k must be [B,Skv,Hkv,D]");
  op.shape(op.dev(v, BF16, "v"), k.sizes(), "v");
  const int Skv = i32(k.size(1)), Hkv = i32(k.size(2));
  TORCH_CHECK(Skv >= 1 && Hkv >= 1 && Hq >= 1 && Hq % Hkv == 0,
              "attn_decode: Skv >= 1, Hq % Hkv (GQA group)");
  auto dense_kv = [&](const Tensor& t, const char* n) {
    TORCH_CHECK(t.stride(3) == 1 && t.stride(2) == D &&
                t.stride(1) == (long)Hkv * D, n, " must be s/h/d-dense");
    if (B > 1) op.dense(t, BF16, n);
  };
  dense_kv(k, "k");
  dense_kv(v, "v");
  op.aligned16("q, k, v", {q.data_ptr(), k.data_ptr(), v.data_ptr()});
  const int* ld = op.opt<int>(len_dev, I32, "len_dev");
  TORCH_CHECK(!ld || len_dev->numel() == 1 || len_dev->numel() == B,
              "len_dev must be [1] or [B]");
  const int len_stride = ld && len_dev->numel() > 1;
  auto o = torch::empty_like(q);
  auto lse = torch::empty({B, Hq, 1}, q.options().dtype(F32));
  if (B == 0) return {o, lse};
  auto part = torch::empty({(long)B * Hq, attn_decode_nsplit(Skv), D + 2},
                           lse.options());
  launch_attn_decode(q.data_ptr(), k.data_ptr(), v.data_ptr(), ld,
                     part.data_ptr<float>(), o.data_ptr(),
                     lse.data_ptr<float>(), B, Hq, Hkv, Skv, D,
                     (float)scale, len_stride, op.stream);
  return {o, lse};
}

// All BSHD, read in place: nothing is transposed on the host side.
std::vector<Tensor> attn_bwd(Tensor q, Tensor k, Tensor v, Tensor o,
                             Tensor dO, Tensor lse, bool causal,
                             double scale, OptTensor doc_start,
                             OptTensor doc_end) {
  const Op op("attn_bwd", q, BF16, "q");
  const AttnShape a = check_attn(op, q, k, v);
  op.shape(op.dense(o, BF16, "o"), q.sizes(), "o");
  op.shape(op.dev(dO, BF16, "dO"), q.sizes(), "dO");
  auto dO_c = dO.contiguous();   // autograd may hand over a strided view
  op.shape(op.dense(lse, F32, "lse"), {a.B, a.Hq, a.S}, "lse");
  op.aligned16("o, dO", {o.data_ptr(), dO_c.data_ptr()});
  const int* dsp = doc_map(op, doc_start, a.B, a.S, "doc_start");
  const int* dep = doc_map(op, doc_end, a.B, a.S, "doc_end");
  TORCH_CHECK((dsp == nullptr) == (dep == nullptr),
              "doc_start and doc_end go together");
  if (dsp) check_docs_shape(causal, a.S, a.Skv);
  // dkdv and dq gather their B-fragments from the ROW-major LDS tiles
  // with ds_read_b64_tr_b16 (tr_bfrag) — no pre-transposed Q/K/dO
  // copies, no transpose_sd pre-passes in the backward at all
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(v);
  if (a.B == 0) return {dq, dk, dv};
  auto delta = torch::empty_like(lse);
  // dq goes first: its prologue forms delta = rowsum(dO o O) from the dO
  // fragments it holds and writes it; dkdv, next on the same stream,
  // reads it. There is no separate delta pass.
  launch_attn_bwd_dq(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                     dO_c.data_ptr(), o.data_ptr(), lse.data_ptr<float>(),
                     delta.data_ptr<float>(), dq.data_ptr(), dsp, a.B, a.Hq,
                     a.Hkv, a.S, a.Skv, a.D, (float)scale, causal ? 1 : 0,
                     op.stream);
  launch_attn_bwd_dkdv(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                       dO_c.data_ptr(), lse.data_ptr<float>(),
                       delta.data_ptr<float>(), dk.data_ptr(),
                       dv.data_ptr(), dep, a.B, a.Hq, a.Hkv, a.S, a.Skv,
                       a.D, (float)scale, causal ? 1 : 0, op.stream);
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
