"""Op dispatch: hand-written gfx950 HIP kernels on GPU, torch reference on CPU.

Policy (deliberate, see repo docs): on a GPU box the in-tree HIP extension
`_dtx_hip` is REQUIRED — any op called with CUDA(=HIP) tensors raises if the
extension failed to import, rather than silently falling back to eager
PyTorch. CPU tensors always use the fp32 torch reference implementations
(tests, plumbing configs).
"""

from __future__ import annotations

import os

import torch

from . import reference as ref

_EXT = None
_EXT_ERR: str | None = None


def _load_ext():
    global _EXT, _EXT_ERR
    if _EXT is not None or _EXT_ERR is not None:
        return _EXT
    try:
        from . import _dtx_hip  # built in-tree by setup.py build_ext --inplace
        _EXT = _dtx_hip
    except Exception as e:  # pragma: no cover - exercised on GPU boxes
        _EXT_ERR = f"{type(e).__name__}: {e}"
    return _EXT


def have_ext() -> bool:
    return _load_ext() is not None


def _gpu(*tensors) -> bool:
    t = tensors[0]
    if not t.is_cuda:
        return False
    ext = _load_ext()
    if ext is None:
        raise RuntimeError(
            "datatunerx_amd HIP extension (_dtx_hip) is not built but a GPU "
            f"tensor reached the op layer. Build it with `python setup.py "
            f"build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950). Import error: "
            f"{_EXT_ERR}")
    return True


# --------------------------------------------------------------- RMSNorm
def rmsnorm_fwd(x, w, eps: float = 1e-5):
    if _gpu(x):
        return _EXT.rmsnorm_fwd(x, w, eps)
    return ref.rmsnorm_fwd(x, w, eps)


def rmsnorm_bwd(dy, x, w, inv, dres=None):
    """dres: optional residual-branch gradient accumulated into dx
    IN-KERNEL (the fused residual+rmsnorm backward — kills the autograd
    grad-accumulation adds on every decoder-layer residual)."""
    if _gpu(x):
        return _EXT.rmsnorm_bwd(dy, x, w, inv, dres)
    dx, dw = ref.rmsnorm_bwd(dy, x, w, inv)
    if dres is not None:
        dx = dx + dres
    return dx, dw


# ------------------------------------------------------------------ RoPE
rope_tables = ref.rope_tables


def _check_doc_start(doc_start, *others):
    """Sequence packing: doc_start excludes the serving-side arguments."""
    if doc_start is None:
        return
    if any(o is not None for o in others):
        raise ValueError("doc_start cannot be combined with len_dev or "
                         "pos_dev")
    if doc_start.dtype != torch.int32:
        raise ValueError("doc_start must be int32")


doc_end_from_start = ref.doc_end_from_start


def rope_fwd(x, cos, sin, pos0: int = 0, pos_dev=None, doc_start=None):
    """doc_start[B,S] (sequence packing): positions restart per document,
    token s sits at pos0 + s - doc_start[b,s]."""
    _check_doc_start(doc_start, pos_dev)
    if _gpu(x):
        return _EXT.rope(x, cos, sin, pos0, False, pos_dev, doc_start)
    if doc_start is not None:
        return ref.rope_fwd(x, cos, sin, pos0, doc_start)
    if pos_dev is not None and pos_dev.numel() > 1:
        # batched ragged decode: per-row positions
        return torch.cat([ref.rope_fwd(x[i:i + 1], cos, sin,
                                       pos0 + int(p))
                          for i, p in enumerate(pos_dev)], dim=0)
    if pos_dev is not None:
        pos0 = pos0 + int(pos_dev)
    return ref.rope_fwd(x, cos, sin, pos0)


def rope_bwd(dy, cos, sin, pos0: int = 0, doc_start=None):
    _check_doc_start(doc_start)
    if _gpu(dy):
        return _EXT.rope(dy, cos, sin, pos0, True, None, doc_start)
    return ref.rope_bwd(dy, cos, sin, pos0, doc_start)


# ---------------------------------------------------------------- SwiGLU
def swiglu_fwd(gate, up):
    if _gpu(gate):
        return _EXT.swiglu_fwd(gate, up)
    return ref.swiglu_fwd(gate, up)


def swiglu_bwd(dout, gate, up):
    if _gpu(gate):
        return _EXT.swiglu_bwd(dout, gate, up)
    return ref.swiglu_bwd(dout, gate, up)


# ------------------------------------------------------ cross entropy
def softmax_xent_fwd(logits, targets, ignore_index: int = -100):
    if _gpu(logits):
        return _EXT.xent_fwd(logits, targets, ignore_index)
    return ref.softmax_xent_fwd(logits, targets, ignore_index)


def softmax_xent_bwd(logits, targets, lse, dloss, ignore_index: int = -100):
    if _gpu(logits):
        return _EXT.xent_bwd(logits, targets, lse, dloss, ignore_index)
    return ref.softmax_xent_bwd(logits, targets, lse, dloss, ignore_index)


def xent_lse_merge(logits_c, targets, m_run, l_run, tgt, v0: int,
                   ignore_index: int = -100):
    if _gpu(logits_c):
        _EXT.xent_lse_merge(logits_c, targets, m_run, l_run, tgt, v0,
                            ignore_index)
        return
    ref.xent_lse_merge(logits_c, targets, m_run, l_run, tgt, v0,
                       ignore_index)


def xent_dlogits(logits_c, targets, lse, v0: int,
                 ignore_index: int = -100):
    if _gpu(logits_c):
        return _EXT.xent_dlogits(logits_c, targets, lse, v0, ignore_index)
    return ref.xent_dlogits(logits_c, targets, lse, v0, ignore_index)


# --------------------------------------------------------- attention
def attn_fwd(q, k, v, causal: bool = True, scale: float | None = None,
             len_dev=None, doc_start=None):
    """BSHD: q [B,S,Hq,D], k/v [B,Skv,Hkv,D] -> (o [B,S,Hq,D], lse).

    doc_start[B,S] int32 (sequence packing): kv row j is visible to q row
    i iff doc_start[i] <= j <= i. Needs causal, S == Skv, S > 1 and no
    len_dev."""
    if scale is None:
        scale = 1.0 / (q.shape[-1] ** 0.5)
    if doc_start is not None:
        _check_doc_start(doc_start, len_dev)
        ref.check_docs(doc_start, causal, q.shape[1], k.shape[1])
        if _gpu(q):
            return _EXT.attn_fwd(q, k, v.contiguous(), causal, scale,
                                 doc_start)
        return ref.attn_fwd(q, k, v, causal, scale, doc_start)
    if _gpu(q):
        if q.shape[1] == 1:
            # serving decode: flash-decoding split-KV path (with S=1
            # every cached position is visible, causal or not).
            # len_dev: device-resident cache length (hipGraph decode).
            return _EXT.attn_decode(q, k, v, scale, len_dev)
        # V consumed row-major (PV B-frags via ds_read_b64_tr_b16):
        # no V pre-transpose
        return _EXT.attn_fwd(q, k, v.contiguous(), causal, scale)
    if len_dev is not None and len_dev.numel() > 1:
        # batched ragged decode on CPU: per-row cache lengths
        outs, lses = [], []
        for i in range(q.shape[0]):
            n = int(len_dev[i])
            o, ls = ref.attn_fwd(q[i:i + 1], k[i:i + 1, :n],
                                 v[i:i + 1, :n], causal, scale)
            outs.append(o)
            lses.append(ls)
        return torch.cat(outs, 0), torch.cat(lses, 0)
    if len_dev is not None:
        k = k[:, :int(len_dev)]
        v = v[:, :int(len_dev)]
    return ref.attn_fwd(q, k, v, causal, scale)


def attn_bwd(q, k, v, o, do, lse, causal: bool = True,
             scale: float | None = None, doc_start=None, doc_end=None):
    """doc_start / doc_end [B,S] int32 (sequence packing): doc_end is
    derived from doc_start when the caller has not done so already."""
    if scale is None:
        scale = 1.0 / (q.shape[-1] ** 0.5)
    if doc_start is not None:
        _check_doc_start(doc_start)
        ref.check_docs(doc_start, causal, q.shape[1], k.shape[1])
        if not _gpu(q):
            return ref.attn_bwd(q, k, v, o, do, lse, causal, scale,
                                doc_start)
        if doc_end is None:
            doc_end = ref.doc_end_from_start(doc_start)
        return _EXT.attn_bwd(q, k, v, o, do, lse, causal, scale, doc_start,
                             doc_end)
    if _gpu(q):
        return _EXT.attn_bwd(q, k, v, o, do, lse, causal, scale)
    return ref.attn_bwd(q, k, v, o, do, lse, causal, scale)


def gemv(x, w):
    """y[...,1,N] = x[...,1,K] @ w[N,K]^T — decode GEMV (single row)."""
    if _gpu(x):
        return _EXT.gemv(x, w)
    return torch.nn.functional.linear(x, w)


def gemm_nt_supported(n: int, k: int) -> bool:
    """Shapes the hand-written MFMA GEMM handles (all Llama projection /
    lm_head shapes); anything else falls back to hipBLASLt."""
    return n % 256 == 0 and k % 64 == 0 and k >= 128


def gemm_nt(a, b, src=None):
    """C[...,N] = a[...,K] @ b[N,K]^T (+ src) via the hand-written
    256x256 MFMA kernel (gemm.hip). bf16 in/out, fp32 accumulate."""
    if _gpu(a):
        return _EXT.gemm_nt(a, b, src)
    out = (a.float() @ b.float().t()).to(a.dtype)
    if src is not None:
        out = out + src.reshape(out.shape)
    return out


# -------------------------------------------------------------- LoRA
# Dropout enters the kernels one of two ways:
#   - `mask`: a materialized bf16 mask tensor (same shape as x / y)
#   - `seed` + `keep` < 1: counter-based RNG computed INSIDE the
#     kernels (splitmix64 on the element offset) — the mask is never
#     written to or read from HBM. The same (seed, offset) yields the
#     same bits in contract/wgrad/expand, so fwd and bwd agree.
def lora_contract(x, w, mask=None, seed: int = 0, keep: float = 1.0):
    if _gpu(x):
        return _EXT.lora_contract(x, w, mask, seed, keep)
    return ref.lora_contract(x, w, mask, seed, keep)


def lora_expand_add(y, t, w, scale: float, mask=None, seed: int = 0,
                    keep: float = 1.0):
    """lora_expand_add_t for an adapter in the PEFT layout, w [N,r]."""
    if _gpu(y):
        return lora_expand_add_t(y, t, w.t().contiguous(), scale, mask,
                                 seed, keep)
    return ref.lora_expand_add(y, t, w, scale, mask, seed, keep)


def lora_wgrad(t, x, scale: float = 1.0, mask=None, seed: int = 0,
               keep: float = 1.0):
    if _gpu(x):
        return _EXT.lora_wgrad(t, x, scale, mask, seed, keep)
    return ref.lora_wgrad(t, x, scale, mask, seed, keep)


# Dual forms: two adapters that share one activation (the q and v LoRA
# pairs of an attention input) in ONE pass over it. Seed-mode dropout
# only, one seed per adapter. Adapters come in the layout the kernels
# read: w0/w1 and a0/a1 are [r,K] / [r,N] (native lora_A; lora_B
# transposed once by the caller).
def lora_contract2(x, w0, w1, seed0: int = 0, seed1: int = 0,
                   keep: float = 1.0):
    """(t0, t1), each bit-identical to lora_contract(x, w, None, seed,
    keep) with its own adapter and seed."""
    if _gpu(x):
        if w0.shape[0] <= 16:
            return tuple(_EXT.lora_contract2(x, w0, w1, seed0, seed1, keep))
        return (_EXT.lora_contract(x, w0, None, seed0, keep),
                _EXT.lora_contract(x, w1, None, seed1, keep))
    return ref.lora_contract2(x, w0, w1, seed0, seed1, keep)


def lora_expand_add_t(y, t, wt, scale: float, mask=None, seed: int = 0,
                      keep: float = 1.0):
    """In place: y[M,N] += (mask o) scale * t[M,r] @ wt[r,N].

    The one place that picks the dropout mode of the expand-add on the
    GPU: seed mode runs in the kernel where it has an RNG mode
    (lora_expand_rng_ok); for the other shapes the same bits are
    materialized with dropout_mask and the kernel runs in mask mode."""
    if _gpu(y):
        N = y.shape[-1]
        M = y.numel() // N
        if (mask is None and keep < 1.0
                and not _EXT.lora_expand_rng_ok(M, N, wt.shape[0])):
            mask, seed, keep = dropout_mask(M, N, seed, keep, y), 0, 1.0
        _EXT.lora_expand_add_t(y, t, wt, scale, mask, seed, keep)
        return y
    return ref.lora_expand_add_t(y, t, wt, scale, mask, seed, keep)


def lora_expand_add2(y, t0, t1, a0, a1, scale: float, seed0: int = 0,
                     seed1: int = 0, keep: float = 1.0):
    """In place: y += mask0 o (s * t0 @ a0) + mask1 o (s * t1 @ a1), one
    read-modify-write and one rounding of y (r <= 16, N % 8 == 0)."""
    if _gpu(y):
        _EXT.lora_expand_add2(y, t0, t1, a0, a1, scale, seed0, seed1, keep)
        return y
    return ref.lora_expand_add2(y, t0, t1, a0, a1, scale, seed0, seed1,
                                keep)


def dropout_mask(M: int, K: int, seed: int, keep: float, like):
    """Materialize the RNG mask (bit-identical to the fused kernels'
    in-kernel bits) — tests and the expand-add shapes without an RNG
    mode (lora_expand_add_t)."""
    if _gpu(like):
        return _EXT.dropout_mask(M, K, seed, keep, like)
    return ref.dropout_mask(M, K, seed, keep, device=like.device,
                            dtype=torch.bfloat16)


# ------------------------------------------- multi-adapter decode LoRA
MLORA_MAX_ROWS = 16
MLORA_RANKS = (8, 16, 32, 64)


def mlora_supported(M: int, N: int, K: int, R: int) -> bool:
    """Shapes the gathered LoRA kernels take (mlora.hip): at most 16
    decode rows, K and N in whole 16-byte bf16 pieces, and a stack rank
    of 8, 16, 32 or 64 (smaller ranks are zero-padded into the stack)."""
    return (1 <= M <= MLORA_MAX_ROWS and K >= 8 and K % 8 == 0
            and N >= 8 and N % 8 == 0 and R in MLORA_RANKS)


def mlora_add(y, x, A, Bt, scale, idx):
    """In place on y [M,N]: y[m] += scale[g] * (x[m] @ A[g]^T) @ Bt[g]
    with g = idx[m]; rows with idx outside [0,G) keep their bits.
    A [G,R,K], Bt [G,R,N] (B pre-transposed), scale [G] f32, idx [M]
    int32 on y's device. On the GPU idx is read by the kernels only (no
    host sync: hipGraph-capturable). There is no fallback in here:
    callers check mlora_supported first, anything else raises."""
    if not (y.dim() == 2 and x.dim() == 2 and A.dim() == 3
            and Bt.dim() == 3):
        raise ValueError("mlora_add: y [M,N], x [M,K], A [G,R,K], "
                         "Bt [G,R,N]")
    M, K = x.shape
    N = y.shape[1]
    G, R = A.shape[0], A.shape[1]
    if not (y.shape[0] == M and A.shape[2] == K
            and tuple(Bt.shape) == (G, R, N) and scale.numel() == G
            and idx.numel() == M):
        raise ValueError(
            f"mlora_add: shape mismatch (y {tuple(y.shape)}, x "
            f"{tuple(x.shape)}, A {tuple(A.shape)}, Bt {tuple(Bt.shape)}, "
            f"scale {tuple(scale.shape)}, idx {tuple(idx.shape)})")
    if not mlora_supported(M, N, K, R):
        raise ValueError(
            f"mlora_add: M={M} N={N} K={K} R={R} is outside the kernel "
            "contract (see mlora_supported)")
    if _gpu(y):
        if not (y.dtype == x.dtype == A.dtype == Bt.dtype == torch.bfloat16
                and scale.dtype == torch.float32
                and idx.dtype == torch.int32 and idx.is_cuda
                and all(t.is_contiguous() and t.data_ptr() % 16 == 0
                        for t in (y, x, A, Bt))
                and scale.is_contiguous() and idx.is_contiguous()):
            raise ValueError(
                "mlora_add: GPU tensors must be contiguous 16-byte-aligned "
                "bf16 (y, x, A, Bt), f32 scale and int32 device idx")
        _EXT.mlora_add(y, x, A, Bt, scale, idx)
        return y
    return ref.mlora_add(y, x, A, Bt, scale, idx)


# ------------------------------------------------------------ sampling
def sample(logits, temperature, top_p, top_k, seed, offset, u=None):
    """One token per row of logits [B, V], each row with its own
    temperature / top_p (fp32 [B]), top_k (int32 [B]) and RNG stream
    (seed int64 [B], offset int32 [B]: the row's token counter) -> int64
    [B]. The contract is ref.sample's; u (fp32 [B] in [0, 1)) replaces
    the RNG. On the GPU everything is read by the kernel only (no host
    sync: hipGraph-capturable); logits must be bf16 with V % 8 == 0, a
    row stride % 8 == 0 and V <= sample_max_vocab()."""
    if _gpu(logits):
        # the binding checks the contract and refuses the rest
        return _EXT.sample(logits, temperature, top_p, top_k, seed, offset,
                           u)
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("sample: logits must be [B, V] with dense rows")
    B = logits.shape[0]
    for name, t, dt in (("temperature", temperature, torch.float32),
                        ("top_p", top_p, torch.float32),
                        ("top_k", top_k, torch.int32),
                        ("seed", seed, torch.int64),
                        ("offset", offset, torch.int32),
                        ("u", u, torch.float32)):
        if t is None and name == "u":
            continue
        if not (tuple(t.shape) == (B,) and t.dtype == dt
                and t.device == logits.device):
            raise ValueError(
                f"sample: {name} must be {dt} [{B}] on the logits' device, "
                f"got {t.dtype} {tuple(t.shape)} on {t.device}")
    return ref.sample(logits, temperature, top_p, top_k, seed, offset, u)


def sample_max_vocab() -> int:
    """Widest row the sampling kernel holds in registers."""
    return 19 * 8 * 1024


# -------------------------------------------------- weight dequant
def dequant_int8(q, scale):
    if _gpu(q):
        return _EXT.dequant_int8(q, scale)
    return (q.float() * scale[:, None]).to(torch.bfloat16)


def dequant_int4(packed, scale, group: int = 64):
    if _gpu(packed):
        return _EXT.dequant_int4(packed, scale, group)
    from ..models.quant import dequantize_int4
    return dequantize_int4(packed, scale, torch.bfloat16, group)


# ------------------------------------------- quantized decode linear
QLINEAR_MAX_ROWS = 16


def qlinear_supported(M: int, N: int, K: int, bits: int,
                      group: int = 64) -> bool:
    """Shapes the weight-streaming qgemv kernels take (qgemv.hip): at
    most 16 rows, and a K that splits into whole 16-byte weight pieces
    (each int4 piece inside one scale group). Anything else goes through
    dequantize-then-linear."""
    if not (1 <= M <= QLINEAR_MAX_ROWS and N >= 1 and K >= 1):
        return False
    if bits == 8:
        return K % 16 == 0
    if bits == 4:
        return K % 32 == 0 and group > 0 and group % 32 == 0 and \
            K % group == 0
    return False


def qlinear(x, qweight, scale, bits: int, group: int = 64):
    """y[...,N] = x[...,K] @ dequant(qweight)[N,K]^T for the weight
    formats of models/quant.py (bits 8: q [N,K] int8 + scale [N];
    bits 4: packed [N,K/2] uint8 + scale [N,K/group]).

    GPU: the qgemv kernels stream the integer weight and dequantize in
    registers when the contract holds (bf16 contiguous x, <= 16 rows,
    qlinear_supported); otherwise the dequant kernel + F.linear. CPU:
    the fp32 reference."""
    if bits not in (4, 8):
        raise ValueError(f"qlinear: bits must be 4 or 8, got {bits}")
    N = qweight.shape[0]
    K = qweight.shape[1] * (2 if bits == 4 else 1)
    if _gpu(x):
        M = x.numel() // K if K else 0
        if (x.dtype == torch.bfloat16 and x.shape[-1] == K
                and x.is_contiguous() and qweight.is_contiguous()
                and scale.is_contiguous()
                and qlinear_supported(M, N, K, bits, group)
                and x.data_ptr() % 16 == 0
                and qweight.data_ptr() % 16 == 0):
            if bits == 8:
                return _EXT.qgemv_int8(x, qweight, scale)
            return _EXT.qgemv_int4(x, qweight, scale, group)
        w = (dequant_int8(qweight, scale) if bits == 8
             else dequant_int4(qweight, scale, group))
        return torch.nn.functional.linear(x, w.to(x.dtype))
    from ..models.quant import dequantize_int4, dequantize_int8
    w = (dequantize_int8(qweight, scale, torch.float32) if bits == 8
         else dequantize_int4(qweight, scale, torch.float32, group))
    return (x.float() @ w.t()).to(x.dtype)


# ------------------------------------------------------------- AdamW
def adamw_step(p_bf16, master, grad, m, v, lr, beta1, beta2, eps,
               weight_decay, step: int):
    if _gpu(master):
        _EXT.adamw(p_bf16, master, grad, m, v, lr, beta1, beta2, eps,
                   weight_decay, step)
        return
    ref.adamw_step(p_bf16, master, grad, m, v, lr, beta1, beta2, eps,
                   weight_decay, step)


def l2_norm(flat):
    if _gpu(flat):
        return _EXT.l2_norm(flat)
    return ref.l2_norm(flat)
