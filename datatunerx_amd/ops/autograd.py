"""torch.autograd.Function wrappers over the fused ops.

These are what the model code calls; each routes to the HIP kernel on GPU
and the torch reference on CPU via datatunerx_amd.ops dispatch.
"""

from __future__ import annotations

import os

import torch

from . import (attn_bwd, attn_fwd, gemm_fp8_nt, gemm_nt_add, lora_contract,
               lora_contract2, lora_expand_add2, lora_expand_add_t,
               lora_wgrad, quant_fp8_rows, rmsnorm_bwd, rmsnorm_fwd, rope_bwd,
               rope_fwd,
               skinny_decode_rows, skinny_linear, skinny_linear_multi,
               softmax_xent_bwd, softmax_xent_fwd, swiglu_bwd, swiglu_fwd)


class RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, eps):
        y, inv = rmsnorm_fwd(x, w, eps)
        ctx.save_for_backward(x, w, inv)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, inv = ctx.saved_tensors
        dx, dw = rmsnorm_bwd(dy.contiguous(), x, w, inv)
        return dx, dw.to(w.dtype), None


def rmsnorm(x, w, eps: float = 1e-5):
    return RMSNorm.apply(x, w, eps)


class ResidualTapRMSNorm(torch.autograd.Function):
    """(norm(x), x) in one node: the layer uses output 1 as the residual
    branch, so x has ONE autograd consumer and the two branch gradients
    merge inside the rmsnorm_bwd kernel instead of a separate
    grad-accumulation add per residual (round-1 STATUS note: ~128 such
    adds/step)."""

    @staticmethod
    def forward(ctx, x, w, eps):
        y, inv = rmsnorm_fwd(x, w, eps)
        ctx.save_for_backward(x, w, inv)
        return y, x

    @staticmethod
    def backward(ctx, dy, dres):
        x, w, inv = ctx.saved_tensors
        from . import rmsnorm_bwd as _bwd
        dx, dw = _bwd(dy.contiguous(), x, w, inv,
                      dres.contiguous() if dres is not None else None)
        return dx, dw.to(w.dtype), None


def rmsnorm_tap(x, w, eps: float = 1e-5):
    return ResidualTapRMSNorm.apply(x, w, eps)


class Rope(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cos, sin, pos0, pos_dev, doc_start):
        ctx.save_for_backward(cos, sin)
        ctx.pos0 = pos0
        ctx.doc_start = doc_start
        return rope_fwd(x, cos, sin, pos0, pos_dev, doc_start)

    @staticmethod
    def backward(ctx, dy):
        cos, sin = ctx.saved_tensors
        return (rope_bwd(dy.contiguous(), cos, sin, ctx.pos0,
                         ctx.doc_start),
                None, None, None, None, None)


def rope(x, cos, sin, pos0: int = 0, pos_dev=None, doc_start=None):
    return Rope.apply(x, cos, sin, pos0, pos_dev, doc_start)


class SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate, up):
        ctx.save_for_backward(gate, up)
        return swiglu_fwd(gate, up)

    @staticmethod
    def backward(ctx, dout):
        gate, up = ctx.saved_tensors
        dgate, dup = swiglu_bwd(dout.contiguous(), gate, up)
        return dgate, dup


def swiglu(gate, up):
    return SwiGLU.apply(gate, up)


class Attention(torch.autograd.Function):
    """BSHD flash attention (no transpose copies around the kernel)."""

    @staticmethod
    def forward(ctx, q, k, v, causal, scale, len_dev, doc_start, doc_end):
        q = q.contiguous()
        if not (q.is_cuda and q.shape[1] == 1):
            # decode (S=1) accepts dense KV-cache prefix views; every
            # other path wants contiguous k/v
            k, v = k.contiguous(), v.contiguous()
        o, lse = attn_fwd(q, k, v, causal, scale, len_dev, doc_start)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.causal, ctx.scale = causal, scale
        ctx.doc_start, ctx.doc_end = doc_start, doc_end
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        dq, dk, dv = attn_bwd(q, k, v, o, do.contiguous(), lse,
                              ctx.causal, ctx.scale, ctx.doc_start,
                              ctx.doc_end)
        return dq, dk, dv, None, None, None, None, None


def attention(q, k, v, causal: bool = True, scale: float | None = None,
              len_dev=None, doc_start=None, doc_end=None):
    """q [B,S,Hq,D], k/v [B,Skv,Hkv,D] -> o [B,S,Hq,D].

    doc_start / doc_end [B,S] int32: document-masked attention for packed
    rows (see ops.attn_fwd)."""
    if scale is None:
        scale = 1.0 / (q.shape[-1] ** 0.5)
    return Attention.apply(q, k, v, causal, scale, len_dev, doc_start,
                           doc_end)


class CrossEntropy(torch.autograd.Function):
    """Mean CE over non-ignored targets; logits [N,V], targets [N]."""

    @staticmethod
    def forward(ctx, logits, targets, ignore_index):
        loss, lse = softmax_xent_fwd(logits, targets, ignore_index)
        n_valid = (targets != ignore_index).sum().clamp(min=1)
        ctx.save_for_backward(logits, targets, lse, n_valid)
        ctx.ignore_index = ignore_index
        return loss.sum() / n_valid.float()

    @staticmethod
    def backward(ctx, dloss):
        logits, targets, lse, n_valid = ctx.saved_tensors
        scale = (dloss.float() / n_valid.float()).expand(logits.shape[0])
        dlogits = softmax_xent_bwd(logits, targets, lse, scale.contiguous(),
                                   ctx.ignore_index)
        return dlogits, None, None


def cross_entropy(logits, targets, ignore_index: int = -100):
    return CrossEntropy.apply(logits, targets, ignore_index)


class PerRowCrossEntropy(torch.autograd.Function):
    """UNREDUCED CE: returns the per-row NLL vector [N] (0 on ignored
    rows) through the same fused xent kernels — the building block for
    per-sequence log-probabilities (DPO)."""

    @staticmethod
    def forward(ctx, logits, targets, ignore_index):
        loss, lse = softmax_xent_fwd(logits, targets, ignore_index)
        ctx.save_for_backward(logits, targets, lse)
        ctx.ignore_index = ignore_index
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, targets, lse = ctx.saved_tensors
        dlogits = softmax_xent_bwd(logits, targets, lse,
                                   dloss.float().contiguous(),
                                   ctx.ignore_index)
        return dlogits, None, None


def per_row_cross_entropy(logits, targets, ignore_index: int = -100):
    return PerRowCrossEntropy.apply(logits, targets, ignore_index)


def _quant(t2, f8):
    """The fp8 operand (q, scale) of an activation or gradient [M,K], once
    per node, when the node's weights route to fp8 (`f8`); else None."""
    return quant_fp8_rows(t2.contiguous()) if f8 is not None else None


def _base_gemm(x2, w, custom, f8=None, xq=None, src=None):
    """Base-projection GEMM x2 @ W^T (+ src): the library's forward
    layout, the hand-written MFMA kernel (gemm.hip) when `custom`
    (opt-in), or with f8 = (w8, sw, wt8, swt) and xq = _quant(x2) the
    e4m3 kernel (gemm_fp8.hip), src in its epilogue."""
    from . import gemm_nt
    if f8 is not None:
        return gemm_fp8_nt(xq[0], xq[1], f8[0], f8[1], src)
    assert src is None
    if custom and x2.is_cuda and x2.shape[0] > 0:
        return gemm_nt(x2, w)
    return torch.nn.functional.linear(x2, w)


def _base_dgrad(dy2, w, wt, custom, f8=None, dq=None):
    """dx = dy2 @ W of a frozen W [N,K]. With the cached wt = W^T [K,N]
    it is F.linear(dy2, wt): the same forward-layout GEMM as the forward
    pass (both operands contraction-contiguous) instead of the library's
    slower "NN" form. `custom`: the hand-written NT kernel on wt. f8, dq =
    _quant(dy2): the e4m3 kernel on the quantized W^T."""
    if f8 is not None:
        return gemm_fp8_nt(dq[0], dq[1], f8[2], f8[3])
    if custom and wt is not None and dy2.is_cuda:
        from . import gemm_nt
        return gemm_nt(dy2, wt)
    if wt is not None:
        return torch.nn.functional.linear(dy2, wt)
    return dy2 @ w


def _dgrad_acc(dx, dy2, w, wt, f8=None, dq=None):
    """dx + dy2 @ W in the GEMM epilogue (beta = 1; in place on the bf16
    routes), against the cached W^T when there is one. Returns the sum."""
    if f8 is not None:
        return gemm_fp8_nt(dq[0], dq[1], f8[2], f8[3], dx)
    return dx.addmm_(dy2, w if wt is None else wt.t())


class LoRALinear(torch.autograd.Function):
    """y = x @ W^T + scale * (dropout(x) @ A^T) @ B^T  with frozen W.

    W: [N,K] (frozen base, no wgrad). `wt` = the cached W^T (or None):
    the dgrad dx = dy @ W then runs in the forward layout, see
    _base_dgrad; `custom` routes both base GEMMs through the hand-written
    gfx950 MFMA kernel (ops/hip/gemm.hip) instead of the library; `f8` =
    the weight's cached fp8 operands routes them through the e4m3 kernel
    (_base_gemm), the low-rank kernels still read the bf16 x and dy. When x
    needs no gradient (layer 0 behind a frozen embedding) the base dgrad
    and the dx expand-add are skipped. The
    low-rank path is the fused HIP contract/expand pair. A: [r,K],
    B: [N,r] (HF PEFT adapter layout, the checkpoint-compat contract —
    SURVEY.md §5 Checkpoint/resume). B is transposed once here and the
    copy reused by the backward; A is read as it is.

    PEFT-style input dropout on the low-rank path is (seed, keep < 1):
    the mask is a counter-based function of (seed, element offset) that
    contract, wgrad and expand-add each regenerate in-kernel, so forward
    and backward agree and it never touches HBM. This node does not pick
    a dropout mode; ops.lora_expand_add_t materializes the mask for the
    shapes whose kernel has no RNG mode.
    """

    @staticmethod
    def forward(ctx, x, w, a, b, scale, wt=None, seed=0, keep=1.0,
                custom=False, f8=None):
        xs = x.shape
        x2 = x.reshape(-1, xs[-1])
        if f8 is not None:
            y = _base_gemm(x2, w, custom, f8, _quant(x2, f8))
        elif x2.is_cuda and x2.shape[0] == 1 and keep >= 1.0:
            from . import gemv
            y = gemv(x2, w)                      # decode: streaming GEMV
        elif keep >= 1.0 and skinny_decode_rows(
                x2, 2, not any(ctx.needs_input_grad)):
            y = skinny_linear(x2, w)             # batched decode: 2-16 rows
        else:
            y = _base_gemm(x2, w, custom)
        bt = b.t().contiguous()                  # [r,N]
        t = lora_contract(x2, a, None, seed, keep)   # (x o mask) @ A^T
        lora_expand_add_t(y, t, bt, scale)       # y += s * t @ B^T
        ctx.save_for_backward(x2, w, a, bt, t, wt)
        ctx.meta = (scale, seed, keep, xs, b.dtype, custom, f8)
        return y.reshape(*xs[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w, a, bt, t, wt = ctx.saved_tensors
        s, seed, keep, xs, b_dtype, custom, f8 = ctx.meta
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        dt = lora_contract(dy2, bt)                   # [M,r] = dy @ B
        db = lora_wgrad(t, dy2, s).t().contiguous()   # [r,N] -> B is [N,r]
        da = lora_wgrad(dt, x2, s, None, seed, keep)  # dt^T @ (x o mask)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _base_dgrad(dy2, w, wt, custom, f8, _quant(dy2, f8))
            # dx += mask o (s * dt @ A)
            lora_expand_add_t(dx, dt, a, s, None, seed, keep)
            dx = dx.reshape(xs)
        return (dx, None, da.to(a.dtype), db.to(b_dtype),
                None, None, None, None, None, None)


def lora_linear(x, w, a, b, scale: float, wt=None):
    return LoRALinear.apply(x, w, a, b, scale, wt)


class FrozenGemm(torch.autograd.Function):
    """y = x @ W^T (+ residual) with frozen W: the one node of a frozen
    projection (the lm_head included).

    Forward: F.linear, or with a residual ops.gemm_nt_add — hipBLASLt
    with C != D, so the residual is added in the GEMM epilogue without
    torch.addmm's copy of it into the result. Backward: dx = dy @ W
    against the cached `wt` = W^T when one is given (_base_dgrad); the
    residual's gradient is dy itself. `custom` runs both GEMMs on the
    hand-written MFMA NT kernel instead (needs wt); `f8` runs both, and
    the residual add, on the e4m3 kernel (_base_gemm)."""

    @staticmethod
    def forward(ctx, x, w, wt, residual, custom=False, f8=None):
        xs = x.shape
        x2 = x.reshape(-1, xs[-1])
        r2 = residual.reshape(-1, w.shape[0]).contiguous() \
            if residual is not None else None
        if f8 is not None:
            y = _base_gemm(x2, w, custom, f8, _quant(x2, f8), r2)
        elif custom:
            from . import gemm_nt
            y = gemm_nt(x2, w, r2)
        elif r2 is not None and skinny_decode_rows(
                x2, 2, not any(ctx.needs_input_grad)):
            y = skinny_linear(x2, w, r2)         # batched decode: 2-16 rows
        elif r2 is None:
            y = torch.nn.functional.linear(x2, w)
        elif x2.is_cuda and not (x2.dtype == torch.bfloat16
                                 and x2.shape[0] > 1):
            y = torch.addmm(r2, x2, w.t())
        else:
            y = gemm_nt_add(x2.contiguous(), w, r2)
        ctx.save_for_backward(w, wt)
        ctx.xshape, ctx.has_res, ctx.custom = xs, residual is not None, custom
        ctx.f8 = f8
        return y.reshape(*xs[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        w, wt = ctx.saved_tensors
        dx = None
        if ctx.needs_input_grad[0]:
            dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
            dx = _base_dgrad(dy2, w, wt, ctx.custom, ctx.f8,
                             _quant(dy2, ctx.f8)).reshape(ctx.xshape)
        return dx, None, None, dy if ctx.has_res else None, None, None


class FusedLinearCrossEntropy(torch.autograd.Function):
    """lm_head GEMM fused with cross-entropy by vocab chunking: the
    [M, V] logits tensor is NEVER materialized (SURVEY.md §2.4 row 1:
    "lm_head fused with cross-entropy to skip the logit
    materialization"). Each chunk's logits [M, Vc] stay cache-resident
    between the chunk GEMM and the online-logsumexp / dlogits kernels.

    The mean-CE backward scale (grad_out / n_valid) is a per-call
    SCALAR, so dX (and dW when the head is trainable) are accumulated
    unscaled during a second forward sweep and backward is a single
    multiply — total GEMM work equals the unfused fwd+dgrad pair while
    logits never round-trip HBM.
    """

    CHUNK = int(os.environ.get("DTX_CE_CHUNK", "4096"))
    MBLOCK = int(os.environ.get("DTX_CE_MBLOCK", "8192"))

    @staticmethod
    def forward(ctx, h2, w, targets, ignore_index, need_grads):
        from . import xent_dlogits, xent_lse_merge
        M, V = h2.shape[0], w.shape[0]
        dev = h2.device
        m = torch.full((M,), -3.4e38, device=dev, dtype=torch.float32)
        l = torch.zeros(M, device=dev, dtype=torch.float32)
        tgt = torch.zeros(M, device=dev, dtype=torch.float32)
        ch = FusedLinearCrossEntropy.CHUNK
        mb = FusedLinearCrossEntropy.MBLOCK
        # block over rows TOO: at mb=8192, ch=4096 the chunk logits
        # (64 MB), the dx row-block and the W chunk stay L3-resident
        # across the vocab sweep; without the row block a chunk is
        # ~200 MB and every re-read/accumulate round-trips HBM.
        for r0 in range(0, M, mb):
            hr = h2[r0:r0 + mb]
            tr = targets[r0:r0 + mb]
            for v0 in range(0, V, ch):
                lc = torch.nn.functional.linear(hr, w[v0:v0 + ch])
                xent_lse_merge(lc, tr, m[r0:r0 + mb], l[r0:r0 + mb],
                               tgt[r0:r0 + mb], v0, ignore_index)
        lse = m + l.log()
        valid = targets != ignore_index
        n_valid = valid.sum().clamp(min=1)
        loss = torch.where(valid, lse - tgt,
                           torch.zeros((), device=dev)).sum() \
            / n_valid.float()
        dx = dw = None
        if need_grads:
            dx = torch.zeros_like(h2)
            if w.requires_grad:
                dw = torch.zeros_like(w)
            for r0 in range(0, M, mb):
                hr = h2[r0:r0 + mb]
                tr = targets[r0:r0 + mb]
                lr = lse[r0:r0 + mb]
                dxr = dx[r0:r0 + mb]
                for v0 in range(0, V, ch):
                    wc = w[v0:v0 + ch]
                    lc = torch.nn.functional.linear(hr, wc)
                    dl = xent_dlogits(lc, tr, lr, v0, ignore_index)
                    dxr.addmm_(dl, wc)
                    if dw is not None:
                        dw[v0:v0 + ch].addmm_(dl.t(), hr)
        ctx.save_for_backward(dx, dw, n_valid)
        return loss

    @staticmethod
    def backward(ctx, gout):
        dx, dw, n_valid = ctx.saved_tensors
        s = (gout.float() / n_valid.float()).to(dx.dtype) \
            if dx is not None else None
        return (dx * s if dx is not None else None, None if dw is None
                else dw * s, None, None, None)


def fused_linear_cross_entropy(h2, w, targets, ignore_index: int = -100):
    need = torch.is_grad_enabled() and (h2.requires_grad or
                                        w.requires_grad)
    return FusedLinearCrossEntropy.apply(h2, w, targets, ignore_index,
                                         need)


class PairedFrozenGemm(torch.autograd.Function):
    """(x@Wg^T, x@Wu^T) for two frozen weights sharing one input (the
    MLP gate/up pair): backward ACCUMULATES the two dgrads into one
    buffer with addmm_ (beta=1 GEMM epilogue), eliminating the autograd
    grad-add that a shared input otherwise costs per layer. wgt / wut:
    the cached W^T of each weight or None (_base_dgrad); f8g / f8u: the
    fp8 operands of both weights, or None for both (_base_gemm)."""

    @staticmethod
    def forward(ctx, x, wg, wu, wgt=None, wut=None, f8g=None, f8u=None):
        xs = x.shape
        x2 = x.reshape(-1, xs[-1])
        xq = _quant(x2, f8g)                     # once, shared by gate/up
        g = _base_gemm(x2, wg, False, f8g, xq)
        u = _base_gemm(x2, wu, False, f8u, xq)
        ctx.save_for_backward(wg, wu, wgt, wut)
        ctx.xshape, ctx.f8 = xs, (f8g, f8u)
        n = wg.shape[0]
        return (g.reshape(*xs[:-1], n), u.reshape(*xs[:-1], n))

    @staticmethod
    def backward(ctx, dg, du):
        wg, wu, wgt, wut = ctx.saved_tensors
        f8g, f8u = ctx.f8
        dg2 = dg.reshape(-1, dg.shape[-1])
        du2 = du.reshape(-1, du.shape[-1])
        dx = _base_dgrad(dg2, wg, wgt, False, f8g, _quant(dg2, f8g))
        # accumulate in the GEMM epilogue
        dx = _dgrad_acc(dx, du2, wu, wut, f8u, _quant(du2, f8u))
        return dx.reshape(ctx.xshape), None, None, None, None, None, None


class QKVProj(torch.autograd.Function):
    """q/k/v projections as ONE autograd node (k frozen; q/v LoRA):
    forward runs the three base GEMMs + the fused LoRA low-rank pairs;
    backward accumulates all three dgrads (and the LoRA dx terms, which
    were already in-place) into ONE dx buffer via addmm_ — removing the
    two [M,E] grad-adds autograd inserts per decoder layer for the
    shared attention input.

    The q and v adapters share x: one dual contract in the forward (two
    dropout seeds, one read of x) and one dual expand-add in the
    backward (one read-modify-write and one rounding of dx). The two
    lora_A gradients stay two wgrad calls — a one-pass dual wgrad
    measured slower (profiles/README.md). lora_B is transposed once in
    the forward and the copy reused by the backward; lora_A is read in
    its native [r,K] layout. `f8`: the fp8 operands of (wq, wk, wv), all
    three or None (_base_gemm)."""

    @staticmethod
    def forward(ctx, x, wq, aq, bq, wk, wv, av, bv, scale,
                seed_q, seed_v, keep, wqt=None, wkt=None, wvt=None,
                f8=None):
        xs = x.shape
        x2 = x.reshape(-1, xs[-1])
        if f8 is not None:
            xq = _quant(x2, f8)                  # once, shared by q/k/v
            yq = _base_gemm(x2, wq, False, f8[0], xq)
            yk = _base_gemm(x2, wk, False, f8[1], xq)
            yv = _base_gemm(x2, wv, False, f8[2], xq)
        elif skinny_decode_rows(x2, 1, not any(ctx.needs_input_grad)):
            # decode: the three base GEMMs in one grouped launch
            yq, yk, yv = skinny_linear_multi(x2, [wq, wk, wv])
        else:
            yq = torch.nn.functional.linear(x2, wq)
            yk = torch.nn.functional.linear(x2, wk)
            yv = torch.nn.functional.linear(x2, wv)
        bqt = bq.t().contiguous()                # [r,Nq]
        bvt = bv.t().contiguous()                # [r,Nv]
        tq, tv = lora_contract2(x2, aq, av, seed_q, seed_v, keep)
        lora_expand_add_t(yq, tq, bqt, scale)
        lora_expand_add_t(yv, tv, bvt, scale)
        ctx.save_for_backward(x2, wq, aq, bqt, wk, wv, av, bvt, tq, tv,
                              wqt, wkt, wvt)
        ctx.meta = (scale, seed_q, seed_v, keep, xs, bq.dtype, bv.dtype)
        ctx.f8 = f8 if f8 is not None else (None, None, None)
        return (yq.reshape(*xs[:-1], wq.shape[0]),
                yk.reshape(*xs[:-1], wk.shape[0]),
                yv.reshape(*xs[:-1], wv.shape[0]))

    @staticmethod
    def backward(ctx, dyq, dyk, dyv):
        (x2, wq, aq, bqt, wk, wv, av, bvt, tq, tv,
         wqt, wkt, wvt) = ctx.saved_tensors
        scale, seed_q, seed_v, keep, xs, bq_dtype, bv_dtype = ctx.meta
        dq2 = dyq.reshape(-1, dyq.shape[-1]).contiguous()
        dv2 = dyv.reshape(-1, dyv.shape[-1]).contiguous()
        # LoRA grads
        dtq = lora_contract(dq2, bqt)
        dtv = lora_contract(dv2, bvt)
        dbq = lora_wgrad(tq, dq2, scale).t().contiguous()
        dbv = lora_wgrad(tv, dv2, scale).t().contiguous()
        daq = lora_wgrad(dtq, x2, scale, None, seed_q, keep)
        dav = lora_wgrad(dtv, x2, scale, None, seed_v, keep)
        dx = None
        if ctx.needs_input_grad[0]:
            # x needs no gradient behind a frozen embedding (layer 0):
            # then the three base dgrads and the dx expand-add are not run
            dk2 = dyk.reshape(-1, dyk.shape[-1]).contiguous()
            f8q, f8k, f8v = ctx.f8
            dx = _base_dgrad(dq2, wq, wqt, False, f8q, _quant(dq2, f8q))
            dx = _dgrad_acc(dx, dk2, wk, wkt, f8k, _quant(dk2, f8k))
            dx = _dgrad_acc(dx, dv2, wv, wvt, f8v, _quant(dv2, f8v))
            # low-rank dx terms (expand_add is in-place on dx)
            lora_expand_add2(dx, dtq, dtv, aq, av, scale, seed_q, seed_v,
                             keep)
            dx = dx.reshape(xs)
        return (dx, None, daq.to(aq.dtype),
                dbq.to(bq_dtype), None, None, dav.to(av.dtype),
                dbv.to(bv_dtype), None, None, None, None, None, None, None,
                None)
