"""Plain-PyTorch reference implementations of every hot op.

These are the numerical contract for the hand-written gfx950 HIP kernels
in datatunerx_amd/ops/hip/: each GPU test compares the HIP kernel against
the fp32 version of the op here. They also serve as the CPU compute path
(tests, the GPT-2-small plumbing config) — on a GPU box the HIP extension
is mandatory and these are NOT silently used (see ops/__init__.py).

Workloads mirror what the reference exercises through HF/PEFT/DeepSpeed
(reference: SURVEY.md §2.4; cmd/tuning/train.py:236-280).
"""

from __future__ import annotations

import torch


# ---------------------------------------------------------------- RMSNorm
def rmsnorm_fwd(x: torch.Tensor, w: torch.Tensor, eps: float = 1e-5):
    """y = x * rsqrt(mean(x^2) + eps) * w.  Returns (y, inv_rms[f32])."""
    xf = x.float()
    inv = torch.rsqrt(xf.pow(2).mean(dim=-1) + eps)  # [M]
    y = (xf * inv.unsqueeze(-1)) * w.float()
    return y.to(x.dtype), inv


def rmsnorm_bwd(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor,
                inv: torch.Tensor):
    """Returns (dx, dw[f32]). dw is reduced over all rows."""
    xf, dyf, wf = x.float(), dy.float(), w.float()
    H = xf.shape[-1]
    g = dyf * wf                                     # [M,H]
    # dx = inv*g - inv^3/H * (g·x) * x
    dot = (g * xf).sum(dim=-1, keepdim=True)         # [M,1]
    dx = inv.unsqueeze(-1) * g - (inv.unsqueeze(-1) ** 3 / H) * dot * xf
    dw = (dyf * xf * inv.unsqueeze(-1)).sum(dim=0)
    return dx.to(x.dtype), dw


# ------------------------------------------------------------------- RoPE
def rope_tables(seq_len: int, head_dim: int, base: float = 10000.0,
                device=None, dtype=torch.float32):
    """cos/sin tables [S, D/2] (host-precomputed; GPU kernels load these)."""
    inv_freq = 1.0 / (base ** (torch.arange(0, head_dim, 2,
                                            device=device).float() / head_dim))
    t = torch.arange(seq_len, device=device).float()
    freqs = torch.outer(t, inv_freq)                 # [S, D/2]
    return freqs.cos().to(dtype), freqs.sin().to(dtype)


def doc_end_from_start(doc_start: torch.Tensor) -> torch.Tensor:
    """Sequence packing: doc_start[B,S] (row index of the first token of
    each token's document) -> doc_end[B,S], the exclusive end of it."""
    B, S = doc_start.shape
    idx = torch.arange(S, device=doc_start.device, dtype=doc_start.dtype)
    # is_last[s]: token s closes its document
    is_last = torch.ones(B, S, dtype=torch.bool, device=doc_start.device)
    is_last[:, :-1] = doc_start[:, 1:] != doc_start[:, :-1]
    # the next closing index at or after s, via a reversed running min
    end = torch.where(is_last, idx + 1, torch.full_like(doc_start, S))
    return end.flip(1).cummin(dim=1).values.flip(1).contiguous()


def _rope_cs(cos, sin, pos0, S, D, doc_start):
    """cos/sin broadcastable to [B,S,H,D/2]; positions restart at each
    document when doc_start[B,S] is given."""
    if doc_start is None:
        return (cos[pos0: pos0 + S].float().view(1, S, 1, D // 2),
                sin[pos0: pos0 + S].float().view(1, S, 1, D // 2))
    pos = pos0 + torch.arange(S, device=doc_start.device) - doc_start.long()
    return (cos[pos].float().unsqueeze(2), sin[pos].float().unsqueeze(2))


def rope_fwd(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
             pos0: int = 0, doc_start=None):
    """Llama rotate-half RoPE. x: [B, S, H, D]; cos/sin: [>=pos0+S, D/2].
    doc_start[B,S]: the position of token s is pos0 + s - doc_start[b,s]."""
    B, S, H, D = x.shape
    xf = x.float()
    x1, x2 = xf[..., : D // 2], xf[..., D // 2:]
    c, s = _rope_cs(cos, sin, pos0, S, D, doc_start)
    y1 = x1 * c - x2 * s
    y2 = x2 * c + x1 * s
    return torch.cat([y1, y2], dim=-1).to(x.dtype)


def rope_bwd(dy: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
             pos0: int = 0, doc_start=None):
    """Gradient of rope_fwd = rotation by -theta (transpose of rotation)."""
    B, S, H, D = dy.shape
    df = dy.float()
    d1, d2 = df[..., : D // 2], df[..., D // 2:]
    c, s = _rope_cs(cos, sin, pos0, S, D, doc_start)
    x1 = d1 * c + d2 * s
    x2 = -d1 * s + d2 * c
    return torch.cat([x1, x2], dim=-1).to(dy.dtype)


# ----------------------------------------------------------------- SwiGLU
def swiglu_fwd(gate: torch.Tensor, up: torch.Tensor):
    g = gate.float()
    return (g * torch.sigmoid(g) * up.float()).to(gate.dtype)


def swiglu_bwd(dout: torch.Tensor, gate: torch.Tensor, up: torch.Tensor):
    g, u, d = gate.float(), up.float(), dout.float()
    sig = torch.sigmoid(g)
    silu = g * sig
    dgate = d * u * (sig + silu * (1.0 - sig))
    dup = d * silu
    return dgate.to(gate.dtype), dup.to(up.dtype)


# ----------------------------------------------- fused softmax cross-entropy
def softmax_xent_fwd(logits: torch.Tensor, targets: torch.Tensor,
                     ignore_index: int = -100):
    """Per-row CE with ignore mask. Returns (loss[f32, N], lse[f32, N]).

    loss[i] = lse[i] - logit[i, t_i]  (0 where ignored).
    Matches the reference's -100 masking (cmd/tuning/train.py:50,98-103).
    """
    lf = logits.float()
    lse = torch.logsumexp(lf, dim=-1)
    mask = targets != ignore_index
    safe_t = targets.masked_fill(~mask, 0)
    picked = lf.gather(-1, safe_t.unsqueeze(-1)).squeeze(-1)
    loss = torch.where(mask, lse - picked, torch.zeros_like(lse))
    return loss, lse


def softmax_xent_bwd(logits: torch.Tensor, targets: torch.Tensor,
                     lse: torch.Tensor, dloss: torch.Tensor,
                     ignore_index: int = -100):
    """dlogits = dloss[i] * (softmax - onehot), 0 on ignored rows."""
    lf = logits.float()
    p = torch.exp(lf - lse.unsqueeze(-1))
    mask = (targets != ignore_index)
    safe_t = targets.masked_fill(~mask, 0)
    p.scatter_add_(-1, safe_t.unsqueeze(-1),
                   -torch.ones_like(p[..., :1]))
    p = p * (dloss * mask.float()).unsqueeze(-1)
    return p.to(logits.dtype)


# -------------------------------------------------------- flash attention
def check_docs(doc_start, causal: bool, S: int, Skv: int):
    """doc_start is defined for the training shape only."""
    if doc_start is None:
        return
    if not causal:
        raise ValueError("doc_start requires causal=True")
    if S != Skv:
        raise ValueError("doc_start requires S == Skv")
    if S <= 1:
        raise ValueError("doc_start requires S > 1")
    if tuple(doc_start.shape) != (doc_start.shape[0], S):
        raise ValueError("doc_start must be [B,S]")


def _visible(S: int, Skv: int, causal: bool, doc_start, device):
    """Boolean mask [B or 1, 1, S, Skv] of visible (q, kv) pairs, or None.
    With doc_start: kv row j is visible to q row i iff
    doc_start[i] <= j <= i."""
    if not causal:
        return None
    mask = torch.ones(S, Skv, dtype=torch.bool, device=device).tril(
        diagonal=Skv - S).view(1, 1, S, Skv)
    if doc_start is not None:
        j = torch.arange(Skv, device=device).view(1, 1, 1, Skv)
        mask = mask & (j >= doc_start.long().view(-1, 1, S, 1))
    return mask


def attn_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
             causal: bool = True, scale: float | None = None,
             doc_start=None):
    """BSHD public contract: q [B,S,Hq,D], k/v [B,Skv,Hkv,D].

    Returns (o [B,S,Hq,D], lse [f32, B,Hq,S])."""
    check_docs(doc_start, causal, q.shape[1], k.shape[1])
    o, lse = _attn_fwd_bhsd(q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3),
                            v.permute(0, 2, 1, 3), causal, scale, doc_start)
    return o.permute(0, 2, 1, 3).contiguous(), lse


def attn_bwd(q, k, v, o, do, lse, causal: bool = True,
             scale: float | None = None, doc_start=None):
    """BSHD public contract; returns (dq, dk, dv) in BSHD."""
    check_docs(doc_start, causal, q.shape[1], k.shape[1])
    p = lambda t: t.permute(0, 2, 1, 3)
    dq, dk, dv = _attn_bwd_bhsd(p(q), p(k), p(v), p(o), p(do), lse,
                                causal, scale, doc_start)
    return (p(dq).contiguous(), p(dk).contiguous(), p(dv).contiguous())


def _attn_fwd_bhsd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                   causal: bool = True, scale: float | None = None,
                   doc_start=None):
    """q: [B,Hq,S,D], k/v: [B,Hkv,S,D] (GQA by head repeat).

    Returns (o [B,Hq,S,D], lse [f32, B,Hq,S]). fp32 math.
    """
    B, Hq, S, D = q.shape
    Hkv = k.shape[1]
    if scale is None:
        scale = 1.0 / (D ** 0.5)
    if Hkv != Hq:
        rep = Hq // Hkv
        k = k.repeat_interleave(rep, dim=1)
        v = v.repeat_interleave(rep, dim=1)
    s = torch.einsum("bhqd,bhkd->bhqk", q.float(), k.float()) * scale
    mask = _visible(S, k.shape[2], causal, doc_start, q.device)
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    o = torch.einsum("bhqk,bhkd->bhqd", p, v.float())
    return o.to(q.dtype), lse


def _attn_bwd_bhsd(q, k, v, o, do, lse, causal: bool = True,
                   scale: float | None = None, doc_start=None):
    """Returns (dq, dk, dv) with GQA reduction over repeated heads."""
    B, Hq, S, D = q.shape
    Hkv = k.shape[1]
    if scale is None:
        scale = 1.0 / (D ** 0.5)
    rep = Hq // Hkv
    kk = k.repeat_interleave(rep, dim=1) if Hkv != Hq else k
    vv = v.repeat_interleave(rep, dim=1) if Hkv != Hq else v
    qf, kf, vf, of, dof = (t.float() for t in (q, kk, vv, o, do))
    s = torch.einsum("bhqd,bhkd->bhqk", qf, kf) * scale
    mask = _visible(S, kf.shape[2], causal, doc_start, q.device)
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    p = torch.exp(s - lse.unsqueeze(-1))
    dv = torch.einsum("bhqk,bhqd->bhkd", p, dof)
    dp = torch.einsum("bhqd,bhkd->bhqk", dof, vf)
    delta = (dof * of).sum(dim=-1, keepdim=True)     # [B,H,S,1]
    ds = p * (dp - delta) * scale
    dq = torch.einsum("bhqk,bhkd->bhqd", ds, kf)
    dk = torch.einsum("bhqk,bhqd->bhkd", ds, qf)
    if Hkv != Hq:
        dk = dk.view(B, Hkv, rep, S, D).sum(dim=2)
        dv = dv.view(B, Hkv, rep, S, D).sum(dim=2)
    return dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)


# ------------------------------------------------------------- LoRA pieces
# Optional `mask` mirrors the fused-dropout GPU kernels: the masked
# element enters the product in the INPUT dtype (x*mask rounded once).
def _masked(x, mask):
    if mask is None:
        return x
    return (x * mask).to(x.dtype)


def dropout_mask(M: int, K: int, seed: int, keep: float,
                 device=None, dtype=torch.bfloat16):
    """Bit-exact CPU twin of the GPU counter-based dropout RNG
    (splitmix64 over 4-element groups, 16 random bits/element,
    threshold keep*65536, value = bf16-rounded 1/keep). Lets CPU
    fallbacks and tests reproduce the fused kernels' mask exactly."""
    assert (M * K) % 4 == 0
    n_groups = (M * K) // 4

    def _u(c):                       # unsigned 64-bit const -> torch int64
        return torch.tensor(c - (1 << 64) if c >= (1 << 63) else c,
                            dtype=torch.int64, device=device)

    def _lshr(z, k):                 # logical shift right on int64
        return (z >> k) & ((1 << (64 - k)) - 1)

    g = torch.arange(n_groups, dtype=torch.int64, device=device)
    z = _u(seed & ((1 << 64) - 1)) + g * _u(0x9E3779B97F4A7C15)
    z = z ^ _lshr(z, 30)
    z = z * _u(0xBF58476D1CE4E5B9)
    z = z ^ _lshr(z, 27)
    z = z * _u(0x94D049BB133111EB)
    z = z ^ _lshr(z, 31)
    thr16 = min(65536, int(keep * 65536.0 + 0.5))
    bits = torch.stack([(z >> (16 * i)) & 0xFFFF for i in range(4)], dim=1)
    keepers = bits < thr16
    inv_keep = torch.tensor(1.0 / keep).to(torch.bfloat16).item()
    return (keepers.reshape(M, K).to(dtype) * inv_keep).to(dtype)


def _resolve_mask(mask, seed, keep, shape, device, dtype):
    if mask is not None or keep >= 1.0:
        return mask
    return dropout_mask(shape[0], shape[1], seed, keep, device=device,
                        dtype=dtype)


def lora_contract(x: torch.Tensor, w: torch.Tensor, mask=None,
                  seed: int = 0, keep: float = 1.0):
    """t[M,r] = (x o mask)[M,K] @ w[r,K]^T  (fp32 out). w is HF lora_A
    layout [r,K], or for the dgrad pass w = lora_B transposed."""
    x2 = x.reshape(-1, x.shape[-1])
    mask = _resolve_mask(mask, seed, keep, x2.shape, x.device, x.dtype)
    return _masked(x2, mask).float() @ w.float().t()


def lora_expand_add(y: torch.Tensor, t: torch.Tensor, w: torch.Tensor,
                    scale: float, mask=None, seed: int = 0,
                    keep: float = 1.0):
    """y[M,N] += (mask o) scale * t[M,r] @ w[N,r]^T  (in-place on y).
    HF lora_B layout is [N,r]."""
    y2 = y.reshape(-1, y.shape[-1])
    mask = _resolve_mask(mask, seed, keep, y2.shape, y.device, y.dtype)
    d = scale * (t.float() @ w.float().t())
    if mask is not None:
        d = d * mask.float()
    y2.add_(d.to(y.dtype))
    return y


def mlora_add(y: torch.Tensor, x: torch.Tensor, A: torch.Tensor,
              Bt: torch.Tensor, scale: torch.Tensor, idx: torch.Tensor):
    """Per-row gathered LoRA update, in place on y [M,N]:
    y[m] += scale[g] * (x[m] @ A[g]^T) @ Bt[g] with g = idx[m]; rows
    whose index is outside [0,G) are left untouched. A [G,R,K],
    Bt [G,R,N] (B pre-transposed), scale [G] f32, idx [M] int."""
    G = A.shape[0]
    for m, g in enumerate(idx.tolist()):
        if 0 <= g < G:
            t = x[m].float() @ A[g].float().t()                  # [R]
            d = float(scale[g]) * (t @ Bt[g].float())            # [N]
            y[m] = (y[m].float() + d).to(y.dtype)
    return y


def lora_wgrad(t: torch.Tensor, x: torch.Tensor, scale: float = 1.0,
               mask=None, seed: int = 0, keep: float = 1.0):
    """dW[r,K] = scale * t[M,r]^T @ (x o mask)[M,K]  (fp32)."""
    x2 = x.reshape(-1, x.shape[-1])
    mask = _resolve_mask(mask, seed, keep, x2.shape, x.device, x.dtype)
    return scale * (t.float().t() @ _masked(x2, mask).float())


# Dual forms (two adapters sharing one activation, e.g. the q and v LoRA
# pairs of one attention input): CPU twins of the one-pass GPU ops.
def lora_contract2(x: torch.Tensor, w0: torch.Tensor, w1: torch.Tensor,
                   seed0: int = 0, seed1: int = 0, keep: float = 1.0):
    """(t0, t1) = ((x o mask0) @ w0^T, (x o mask1) @ w1^T): exactly two
    lora_contract calls (the GPU op reads x once)."""
    return (lora_contract(x, w0, None, seed0, keep),
            lora_contract(x, w1, None, seed1, keep))


def lora_expand_add_t(y: torch.Tensor, t: torch.Tensor, wt: torch.Tensor,
                      scale: float, mask=None, seed: int = 0,
                      keep: float = 1.0):
    """lora_expand_add with the adapter already transposed: wt [r,N]."""
    return lora_expand_add(y, t, wt.t(), scale, mask, seed, keep)


def lora_expand_add2(y: torch.Tensor, t0: torch.Tensor, t1: torch.Tensor,
                     a0: torch.Tensor, a1: torch.Tensor, scale: float,
                     seed0: int = 0, seed1: int = 0, keep: float = 1.0):
    """y[M,N] += mask0 o (s * t0 @ a0) + mask1 o (s * t1 @ a1) in place,
    a0/a1 [r,N]. Both terms are summed with y in fp32 and rounded ONCE
    (two lora_expand_add calls round y in between)."""
    y2 = y.reshape(-1, y.shape[-1])
    acc = y2.float()
    for t, a, seed in ((t0, a0, seed0), (t1, a1, seed1)):
        d = scale * (t.float() @ a.float())
        mask = _resolve_mask(None, seed, keep, y2.shape, y.device, y.dtype)
        if mask is not None:
            d = d * mask.float()
        acc = acc + d
    y2.copy_(acc.to(y.dtype))
    return y


# ------------------------------------------------------------ fused AdamW
def adamw_step(p_bf16: torch.Tensor, master: torch.Tensor,
               grad: torch.Tensor, m: torch.Tensor, v: torch.Tensor,
               lr: float, beta1: float, beta2: float, eps: float,
               weight_decay: float, step: int):
    """Single-pass AdamW on flat fp32 master weights; p_bf16 gets the
    rounded copy. Decoupled weight decay (torch AdamW convention)."""
    gf = grad.float()
    m.mul_(beta1).add_(gf, alpha=1.0 - beta1)
    v.mul_(beta2).addcmul_(gf, gf, value=1.0 - beta2)
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    master.mul_(1.0 - lr * weight_decay)
    denom = (v / bc2).sqrt_().add_(eps)
    master.addcdiv_(m, denom, value=-lr / bc1)
    p_bf16.copy_(master.to(p_bf16.dtype))


def l2_norm(flat: torch.Tensor) -> torch.Tensor:
    return flat.float().pow(2).sum().sqrt()


def xent_lse_merge(logits_c, targets, m_run, l_run, tgt, v0: int,
                   ignore_index: int = -100):
    """CPU fp32 reference of the chunked online-LSE merge (in-place)."""
    x = logits_c.float()
    cmax = x.max(dim=-1).values
    csum = (x - cmax[:, None]).exp().sum(dim=-1)
    m_new = torch.maximum(m_run, cmax)
    l_run.mul_((m_run - m_new).exp()).add_(csum * (cmax - m_new).exp())
    m_run.copy_(m_new)
    vc = x.shape[-1]
    inside = (targets != ignore_index) & (targets >= v0) & \
        (targets < v0 + vc)
    idx = inside.nonzero(as_tuple=True)[0]
    if idx.numel():
        tgt[idx] = x[idx, (targets[idx] - v0)]


def xent_dlogits(logits_c, targets, lse, v0: int,
                 ignore_index: int = -100):
    x = logits_c.float()
    dl = (x - lse[:, None]).exp()
    vc = x.shape[-1]
    inside = (targets != ignore_index) & (targets >= v0) & \
        (targets < v0 + vc)
    idx = inside.nonzero(as_tuple=True)[0]
    if idx.numel():
        dl[idx, (targets[idx] - v0)] -= 1.0
    dl[targets == ignore_index] = 0.0
    return dl.to(logits_c.dtype)


# ------------------------------------------------------------- sampling
def sample_rng(seed: torch.Tensor, offset: torch.Tensor) -> torch.Tensor:
    """The sampler's random bits, int64 [B] in [0, 2^24): the splitmix64
    finalizer of dropout_mask over z = seed + (offset + 1) * GAMMA
    (mod 2^64), top 24 bits. Keyed by a row's own (seed, offset) only.
    Integer arithmetic, so it is the GPU kernel's value bit for bit."""
    def _u(c):
        return c - (1 << 64) if c >= (1 << 63) else c

    def _lshr(z, k):
        return (z >> k) & ((1 << (64 - k)) - 1)

    z = seed.to(torch.int64) + (offset.to(torch.int64) + 1) * \
        _u(0x9E3779B97F4A7C15)
    z = z ^ _lshr(z, 30)
    z = z * _u(0xBF58476D1CE4E5B9)
    z = z ^ _lshr(z, 27)
    z = z * _u(0x94D049BB133111EB)
    z = z ^ _lshr(z, 31)
    return _lshr(z, 40)


def sample(logits: torch.Tensor, temperature: torch.Tensor,
           top_p: torch.Tensor, top_k: torch.Tensor, seed: torch.Tensor,
           offset: torch.Tensor, u=None) -> torch.Tensor:
    """fp32 twin of the sampling kernel (sample.hip), every row with its
    own parameters -> int64 [B].

    temperature <= 0: first index of the row maximum. Otherwise, in the
    order (logit descending, index ascending) and with the weights
    w = exp((l - l_max) / temperature): the candidates are the first
    top_k (all when top_k <= 0 or >= V); the nucleus is their longest
    prefix whose weight sum is <= top_p * Z_C (Z_C: the candidates' sum;
    all candidates when top_p >= 1), never fewer than one; the token is
    the first nucleus member, in INDEX order, whose running weight sum
    exceeds u * Z_N (the last member when rounding leaves none). u is
    sample_rng(seed, offset) * 2^-24 unless given."""
    B, V = logits.shape
    if u is None:
        u = sample_rng(seed, offset).to(torch.float32) * (2.0 ** -24)
    x = logits.float()
    T = temperature.float().view(B, 1)
    greedy = ~(T > 0)
    w = torch.exp((x - x.max(1, keepdim=True).values) /
                  torch.where(greedy, torch.ones_like(T), T))
    _, order = torch.sort(x, dim=1, descending=True, stable=True)
    k = top_k.view(B, 1).to(torch.int64)
    k = torch.where((k <= 0) | (k >= V), torch.full_like(k, V), k)
    cand = torch.arange(V, device=x.device).view(1, V) < k
    cum = torch.cumsum(torch.gather(w, 1, order) * cand, dim=1)
    p = top_p.float().view(B, 1)
    keep = cand & ((cum <= p * cum[:, -1:]) | (p >= 1))
    keep[:, 0] = True
    member = torch.zeros_like(keep).scatter_(1, order, keep)
    cdf = torch.cumsum(w * member, dim=1)
    target = u.float().view(B, 1) * cdf[:, -1:]
    hit = member & (cdf > target)
    first = hit.to(torch.int8).argmax(1)
    last = V - 1 - member.flip(1).to(torch.int8).argmax(1)
    tok = torch.where(hit.any(1), first, last)
    return torch.where(greedy.view(B), x.argmax(1), tok)
