"""Op dispatch: hand-written gfx950 HIP kernels on GPU, torch reference on CPU.

Policy (deliberate, see repo docs): on a GPU box the in-tree HIP extension
`_dtx_hip` is REQUIRED — any op called with CUDA(=HIP) tensors raises if the
extension failed to import, rather than silently falling back to eager
PyTorch. CPU tensors always use the fp32 torch reference implementations
(tests, plumbing configs).
"""

from __future__ import annotations

import os
from typing import NamedTuple, Optional

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
            # A GQA model's cache rows are shared by the query heads of
            # their kv head (attn_decode_gqa.hip); MHA keeps its kernel.
            if _gqa_decode_ok(q, k):
                return _EXT.attn_decode_gqa(q, k, v, scale, len_dev)
            return _EXT.attn_decode(q, k, v, scale, len_dev)
        if len_dev is not None:
            # a multi-token step over the cache (speculative verify): the
            # only S > 1 kernel that reads the live length on the device
            if not causal or q.dim() != 4 or k.dim() != 4 or \
                    not _EXT.attn_verify_supported(
                        q.shape[1], q.shape[2], k.shape[2], q.shape[3]):
                raise ValueError(
                    "attn_fwd: S > 1 with len_dev needs causal attention "
                    "inside attn_verify_supported (D 64 or 128, S <= 16, "
                    f"S * Hq / Hkv <= 32), got q {tuple(q.shape)}, "
                    f"k {tuple(k.shape)}")
            return _EXT.attn_verify(q, k, v, scale, len_dev)
        # V consumed row-major (PV B-frags via ds_read_b64_tr_b16):
        # no V pre-transpose
        return _EXT.attn_fwd(q, k, v.contiguous(), causal, scale)
    return _attn_fwd_cpu(q, k, v, causal, scale, len_dev)


def _attn_fwd_cpu(q, k, v, causal, scale, len_dev):
    """The fp32 reference with the serving arguments: len_dev is one cache
    length or one per batch row."""
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


def gqa_decode_supported(Hq: int, Hkv: int, D: int) -> bool:
    """Head shapes the GQA-shared bf16 decode kernel takes
    (attn_decode_gqa.hip): head_dim 64 or 128 and 2 to 16 query heads per
    kv head. The predicate is the extension's own (the one its binding
    checks)."""
    ext = _load_ext()
    if ext is None:
        raise RuntimeError("gqa_decode_supported needs the HIP extension "
                           f"(_dtx_hip): {_EXT_ERR}")
    return bool(ext.gqa_decode_supported(Hq, Hkv, D))


def _gqa_decode_ok(q, k) -> bool:
    """attn_fwd's S == 1 routing, DTX_GQA_DECODE read per call: 0 never,
    1 wherever the kernel applies, unset where it was measured not to
    lose (profiles/README.md, "GQA-shared bf16 decode"): groups above 4,
    and groups up to 4 from a capacity of 8192 rows. At G = 4 and 2048
    rows it lost 23-25 % on short live lengths at B >= 8."""
    knob = os.environ.get("DTX_GQA_DECODE", "")
    if knob == "0" or q.dim() != 4 or k.dim() != 4:
        return False
    Hq, Hkv = q.shape[2], k.shape[2]
    if not _EXT.gqa_decode_supported(Hq, Hkv, q.shape[3]):
        return False
    return knob == "1" or Hq // Hkv > 4 or k.shape[1] >= 8192


def attn_decode_gqa(q, k, v, scale: float | None = None, len_dev=None):
    """Decode attention of q [B,1,Hq,D] over the bf16 KV cache k, v
    [B,Skv,Hkv,D] -> (o [B,1,Hq,D], lse [B,Hq,1]), all query heads of a
    GQA group sharing one pass over their kv head's rows. attn_decode's
    contract (k, v may be the B == 1 prefix view of a larger cache;
    len_dev int32 [1] or [B], read on the device and clamped to Skv);
    needs gqa_decode_supported(Hq, Hkv, D). ops.attn_fwd routes here."""
    if scale is None:
        scale = 1.0 / (q.shape[-1] ** 0.5)
    if _gpu(q):
        return _EXT.attn_decode_gqa(q, k, v, scale, len_dev)
    if q.dim() != 4 or q.shape[1] != 1:
        raise ValueError("attn_decode_gqa: q must be [B,1,Hq,D]")
    if len_dev is not None:
        if len_dev.numel() not in (1, q.shape[0]):
            raise ValueError("attn_decode_gqa: len_dev must be [1] or [B]")
        len_dev = len_dev.clamp(max=k.shape[1])
    return _attn_fwd_cpu(q, k, v, False, scale, len_dev)


def attn_verify_supported(T: int, Hq: int, Hkv: int, D: int) -> bool:
    """Shapes the multi-token verify kernel takes (attn_verify.hip):
    head_dim 64 or 128, Hq % Hkv == 0, 1 <= T <= 16 query rows and
    T * Hq / Hkv <= 32. The predicate is the extension's own (the one its
    binding checks)."""
    ext = _load_ext()
    if ext is None:
        raise RuntimeError("attn_verify_supported needs the HIP extension "
                           f"(_dtx_hip): {_EXT_ERR}")
    return bool(ext.attn_verify_supported(T, Hq, Hkv, D))


def attn_verify(q, k, v, scale: float | None = None, len_dev=None):
    """Attention of the T new tokens of a decode step, q [B,T,Hq,D], over
    the bf16 KV cache k, v [B,cap,Hkv,D] that already holds their rows ->
    (o [B,T,Hq,D], lse [B,Hq,T]). len_dev (int32 [1] or [B], read on the
    device and clamped to cap) is the live length INCLUDING the T rows;
    without it every row of k is live (the B == 1 prefix view). Query t of
    row b sees kv rows j <= len[b] - T + t. A row with fewer than T live
    rows is the caller's error: the kernel gives the queries that see
    nothing o = 0, the CPU reference raises. Needs
    attn_verify_supported(T, Hq, Hkv, D). ops.attn_fwd routes here for
    S > 1 with len_dev."""
    if scale is None:
        scale = 1.0 / (q.shape[-1] ** 0.5)
    if _gpu(q):
        return _EXT.attn_verify(q, k, v, scale, len_dev)
    if q.dim() != 4:
        raise ValueError("attn_verify: q must be [B,T,Hq,D]")
    B, cap = q.shape[0], k.shape[1]
    lens = [cap] * B
    if len_dev is not None:
        if len_dev.numel() not in (1, B):
            raise ValueError("attn_verify: len_dev must be [1] or [B]")
        lens = [min(int(n), cap) for n in len_dev.expand(B).tolist()]
    return ref.attn_verify(q, k, v, scale, lens)


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


# ------------------------------------------------------ int8 KV cache
class KV8(NamedTuple):
    """An int8 KV cache as attn_decode_q8 takes it: k8, v8
    [Bc,max_s,Hkv,D] int8, ks, vs [Bc,Hkv,max_s] f32, and the host-side
    live length (None: len_dev, or the capacity)."""
    k8: torch.Tensor
    v8: torch.Tensor
    ks: torch.Tensor
    vs: torch.Tensor
    length: Optional[int] = None


def kv_int8_supported(Hq: int, Hkv: int, D: int) -> bool:
    """Head shapes the int8 KV kernels take (kvq.hip): head_dim 64 or 128
    and a GQA group of at most 16 query heads per kv head."""
    return (D in (64, 128) and Hkv >= 1 and Hq >= 1 and Hq % Hkv == 0
            and Hq // Hkv <= 16)


def kv_quant_append(k, v, k8, v8, ks, vs, start: int = 0, wpos=None):
    """Quantize k, v [B,S,Hkv,D] row by row (models/quant.py's per-row
    absmax int8) into the cache k8, v8 [Bc,max_s,Hkv,D] int8 with scales
    ks, vs [Bc,Hkv,max_s] f32. Row (b, s) goes to slot (b, start + s); with
    wpos (int64 [B], S == 1) row b goes to the flat slot wpos[b] of
    [Bc * max_s], read on the device (no host sync: hipGraph-capturable),
    and a slot outside the cache is skipped."""
    if _gpu(k):
        _EXT.kv_quant_append(k, v, k8, v8, ks, vs, start, wpos)
        return
    B, S = k.shape[:2]
    if wpos is not None and S != 1:
        raise ValueError("kv_quant_append: wpos needs S == 1")
    if B > k8.shape[0] or (wpos is None and
                           not 0 <= start <= k8.shape[1] - S):
        raise ValueError(f"kv_quant_append: rows {start}..{start + S} of "
                         f"{B} batch rows do not fit the cache "
                         f"{tuple(k8.shape)}")
    ref.kv_quant_append(k, v, k8, v8, ks, vs, start, wpos)


def attn_decode_q8(q, k8, v8, ks, vs, scale: float | None = None,
                   len_dev=None, length: int | None = None):
    """Decode attention of q [B,1,Hq,D] over an int8 KV cache (see
    kv_quant_append) -> (o [B,1,Hq,D], lse [B,Hq,1]). The live length of
    batch row b is len_dev (int32 [1] or [B], read on the device), else
    `length`, else the capacity. All query heads of a GQA group share
    one pass over the cache; needs kv_int8_supported(Hq, Hkv, D)."""
    if scale is None:
        scale = 1.0 / (q.shape[-1] ** 0.5)
    if _gpu(q):
        return _EXT.attn_decode_q8(q, k8, v8, ks, vs, scale, len_dev, length)
    B, Hq, D = q.shape[0], q.shape[2], q.shape[3]
    if not kv_int8_supported(Hq, k8.shape[2], D):
        raise ValueError(f"attn_decode_q8: Hq={Hq} Hkv={k8.shape[2]} D={D} "
                         "is outside the kernel contract "
                         "(see kv_int8_supported)")
    if len_dev is not None and length is not None:
        raise ValueError("attn_decode_q8: give len_dev or length, not both")
    if len_dev is not None:
        if len_dev.numel() not in (1, B):
            raise ValueError("attn_decode_q8: len_dev must be [1] or [B]")
        lens = [min(int(n), k8.shape[1])
                for n in len_dev.expand(B).tolist()]
    else:
        lens = [k8.shape[1] if length is None else int(length)] * B
    return ref.attn_decode_q8(q, k8, v8, ks, vs, scale, lens)


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


def gemm_nt_add(a, b, c):
    """d[M,N] = a[M,K] @ b[N,K]^T + c[M,N], bf16 with fp32 accumulation,
    on hipBLASLt with C != D (basegemm.cpp): c is read and never written,
    d is a fresh tensor. What torch.addmm(c, a, b.t()) computes, without
    its copy of c into the result."""
    if _gpu(a):
        return _EXT.gemm_nt_add(a, b, c)
    return torch.addmm(c, a, b.t())


# ------------------------------------------------------- fp8 base GEMMs
def gemm_fp8_supported(n: int, k: int) -> bool:
    """[N,K] weights the e4m3 MFMA GEMM takes (gemm_fp8.hip): the
    extension's own predicate, the one its binding checks."""
    ext = _load_ext()
    if ext is None:
        raise RuntimeError("gemm_fp8_supported needs the HIP extension "
                           f"(_dtx_hip): {_EXT_ERR}")
    return bool(ext.gemm_fp8_supported(n, k))


def quant_fp8_rows(x):
    """bf16 x [..., K] -> (q e4m3, scale f32 [rows]), one scale per row:
    scale = absmax / 448, q = e4m3(clamp(x / scale)). The GPU kernel and
    the CPU twin give the same bits."""
    if _gpu(x):
        return tuple(_EXT.quant_fp8_rows(x))
    return ref.quant_fp8_rows(x)


def gemm_fp8_nt(a8, sa, b8, sb, src=None):
    """bf16 C[...,N] = sa[m] * sb[n] * (a8[...,K] @ b8[N,K]^T) (+ src) on
    the 128-deep e4m3 MFMA (gemm_fp8.hip): fp32 accumulate, scales and src
    in the fp32 epilogue, one rounding."""
    if _gpu(a8):
        return _EXT.gemm_fp8_nt(a8, sa, b8, sb, src)
    return ref.gemm_fp8_nt(a8, sa, b8, sb, src)


# --------------------------------------------- skinny bf16 decode GEMMs
SKINNY_MAX_ROWS = 16


def skinny_supported(M: int, N: int, K: int) -> bool:
    """Shapes the bf16 weight-streaming kernels take (skinny.hip): 1 to 16
    rows, K in whole 16-byte pieces. The predicate is the extension's own
    (the one its bindings check)."""
    ext = _load_ext()
    if ext is None:
        raise RuntimeError("skinny_supported needs the HIP extension "
                           f"(_dtx_hip): {_EXT_ERR}")
    return bool(ext.skinny_supported(M, N, K))


def _skinny_ok(x, *ws) -> bool:
    """Does the kernel take this call? bf16, dense, 16-byte aligned,
    skinny_supported, and DTX_SKINNY_GEMM != 0."""
    if os.environ.get("DTX_SKINNY_GEMM", "1") == "0":
        return False
    K = x.shape[-1]
    if not (x.dtype == torch.bfloat16 and K > 0 and x.is_contiguous()
            and x.data_ptr() % 16 == 0):
        return False
    M = x.numel() // K
    return all(w.dtype == torch.bfloat16 and w.dim() == 2
               and w.shape[1] == K and w.is_contiguous()
               and w.data_ptr() % 16 == 0 and w.device == x.device
               and _EXT.skinny_supported(M, max(w.shape[0], 1), K)
               for w in ws)


def skinny_decode_rows(x, min_rows: int = 1, no_grad=None) -> bool:
    """Call-site test: a no-grad bf16 GPU activation of min_rows..16 rows,
    the calls the skinny kernels are for (the op still checks the rest).
    no_grad: for autograd nodes, whose forward always runs with grad mode
    off: whether no input of the node needs a gradient."""
    if no_grad is None:
        no_grad = not torch.is_grad_enabled()
    if not no_grad or not x.is_cuda or x.dtype != torch.bfloat16 or \
            x.shape[-1] == 0:
        return False
    return min_rows <= x.numel() // x.shape[-1] <= SKINNY_MAX_ROWS


def skinny_linear(x, w, residual=None):
    """y[...,N] = x[...,K] @ w[N,K]^T (+ residual [...,N]) for decode-sized
    x. GPU: the weight-streaming MFMA kernel where _skinny_ok, else what
    ran before it (F.linear; gemm_nt_add / addmm with a residual)."""
    if _gpu(x):
        N = w.shape[0]
        if _skinny_ok(x, w) and (residual is None or (
                residual.dtype == torch.bfloat16
                and residual.numel() == x.numel() // x.shape[-1] * N)):
            r = None if residual is None else residual.contiguous()
            return _EXT.skinny_gemm(x, w, r)
        if residual is None:
            return torch.nn.functional.linear(x, w)
        x2 = x.reshape(-1, x.shape[-1])
        r2 = residual.reshape(-1, N).contiguous()
        if x2.dtype == torch.bfloat16 and x2.shape[0] > 1:
            y = _EXT.gemm_nt_add(x2.contiguous(), w.contiguous(), r2)
        else:
            y = torch.addmm(r2, x2, w.t())
        return y.reshape(*x.shape[:-1], N)
    return ref.skinny_linear(x, w, residual)


def skinny_linear_multi(x, ws):
    """[x @ w^T for w in ws] for up to three weights that share x (q/k/v):
    one grouped launch, each output bit-identical to skinny_linear(x, w)."""
    ws = list(ws)
    if _gpu(x):
        if 1 <= len(ws) <= 3 and _skinny_ok(x, *ws):
            return list(_EXT.skinny_gemm_multi(x, ws))
        return [torch.nn.functional.linear(x, w) for w in ws]
    return ref.skinny_linear_multi(x, ws)


def skinny_swiglu(x, wg, wu):
    """swiglu(x @ wg^T, x @ wu^T) with the two products rounded to bf16
    as the two-GEMM path stores them; on the kernel path g and u never
    reach HBM."""
    if _gpu(x):
        if wg.shape == wu.shape and _skinny_ok(x, wg, wu):
            return _EXT.skinny_swiglu(x, wg, wu)
        return swiglu_fwd(torch.nn.functional.linear(x, wg).contiguous(),
                          torch.nn.functional.linear(x, wu).contiguous())
    return ref.skinny_swiglu(x, wg, wu)


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


def dequant_nf4(packed, absmax, group: int = 64):
    """bf16(NF4_CODE[idx] * absmax): the GPU kernel and the CPU reference
    give the same bits."""
    if _gpu(packed):
        return _EXT.dequant_nf4(packed, absmax, group)
    from ..models.quant import dequantize_nf4
    return dequantize_nf4(packed, absmax, torch.bfloat16, group)


# ------------------------------------------- quantized decode linear
QLINEAR_MAX_ROWS = 16
# CPU-side copy of quant_fp8_max_k(), read only where the extension is not
# loaded; with it loaded every fp8 shape rule is the extension's predicate
FP8_QUANT_MAX_K = 16384


def qlinear_supported(M: int, N: int, K: int, bits: int,
                      group: int = 64, codebook=None) -> bool:
    """Shapes the weight-streaming qgemv kernels take (qgemv.hip): at
    most 16 rows, and a K that splits into whole 16-byte weight pieces
    (each int4 piece inside one scale group). codebook "e4m3"
    (qgemv_fp8.hip): whole 128-deep k-steps and a row the in-kernel
    quantizer holds, FP8_QUANT_MAX_K. Anything else goes through
    dequantize-then-linear."""
    if not (1 <= M <= QLINEAR_MAX_ROWS and N >= 1 and K >= 1):
        return False
    if codebook == "e4m3":
        if bits != 8:
            return False
        ext = _load_ext()
        if ext is not None:       # the one predicate, the binding's own
            return bool(ext.qgemv_fp8_supported(M, N, K))
        return K % 128 == 0 and K <= FP8_QUANT_MAX_K
    if bits == 8:
        return K % 16 == 0
    if bits == 4:
        return K % 32 == 0 and group > 0 and group % 32 == 0 and \
            K % group == 0
    return False


def _qlinear_fp8(x, w8, sw):
    """The fp8 contract on an e4m3 weight: quant_fp8_rows on x, fp32
    accumulation, both scales in the fp32 epilogue, one rounding. GPU: up
    to 16 rows the weight-streaming kernel (it quantizes x itself), more
    rows the quantizer and the e4m3 MFMA GEMM; only a shape outside both
    kernels dequantizes and multiplies. CPU: the reference twin."""
    N, K = w8.shape
    if not _gpu(x):
        return ref.qlinear_fp8(x, w8, sw)
    M = x.numel() // K if K else 0
    dense = (x.dtype == torch.bfloat16 and x.shape[-1] == K
             and x.is_contiguous() and w8.is_contiguous()
             and sw.is_contiguous() and x.data_ptr() % 16 == 0
             and w8.data_ptr() % 16 == 0)
    if dense and _EXT.qgemv_fp8_supported(M, N, K):
        return _EXT.qgemv_fp8(x, w8, sw)
    if (dense and M > QLINEAR_MAX_ROWS and K <= _EXT.quant_fp8_max_k()
            and _EXT.gemm_fp8_supported(N, K) and sw.data_ptr() % 16 == 0):
        return gemm_fp8_nt(*quant_fp8_rows(x), w8, sw)
    w = (w8.float() * sw[:, None]).to(torch.bfloat16)
    return torch.nn.functional.linear(x, w.to(x.dtype))


def qlinear(x, qweight, scale, bits: int, group: int = 64, codebook=None):
    """y[...,N] = x[...,K] @ dequant(qweight)[N,K]^T for the weight
    formats of models/quant.py (bits 8: q [N,K] int8 + scale [N];
    bits 4: packed [N,K/2] uint8 + scale [N,K/group]; bits 4 with
    codebook "nf4": packed NF4 indices + absmax [N,K/group]; bits 8 with
    codebook "e4m3": q [N,K] e4m3 + scale [N], multiplied under the fp8
    contract, see _qlinear_fp8).

    GPU: the qgemv kernels stream the integer weight and dequantize in
    registers when the contract holds (bf16 contiguous x, <= 16 rows,
    qlinear_supported); otherwise the dequant kernel + F.linear. CPU:
    the fp32 reference."""
    if bits not in (4, 8):
        raise ValueError(f"qlinear: bits must be 4 or 8, got {bits}")
    if codebook not in (None, "nf4", "e4m3") or \
            (codebook and bits != {"nf4": 4, "e4m3": 8}[codebook]):
        raise ValueError(f"qlinear: codebook {codebook!r} with bits={bits}")
    if codebook == "e4m3":
        return _qlinear_fp8(x, qweight, scale)
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
            if codebook == "nf4":
                return _EXT.qgemv_nf4(x, qweight, scale, group)
            return _EXT.qgemv_int4(x, qweight, scale, group)
        w = (dequant_int8(qweight, scale) if bits == 8
             else dequant_nf4(qweight, scale, group) if codebook == "nf4"
             else dequant_int4(qweight, scale, group))
        return torch.nn.functional.linear(x, w.to(x.dtype))
    from ..models.quant import (dequantize_int4, dequantize_int8,
                                dequantize_nf4)
    w = (dequantize_int8(qweight, scale, torch.float32) if bits == 8
         else dequantize_nf4(qweight, scale, torch.float32, group)
         if codebook == "nf4"
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
