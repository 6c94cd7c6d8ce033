"""Row-wise error bounds for the kernel tests (docs/kernels.md, "Numerics
bounds"). A plain helper module: the tests import it by name, the way
free_port is imported from conftest.

Three things live here.

fp64 references. The inputs are the bf16 (or fp32) tensors the kernel gets;
all math runs in float64 on the CPU. ops/reference.py is the fp32 twin that
production CPU paths run; these exist only to be more precise than it.

A magnitude budget beside each result: the same sum with every term replaced
by its absolute value, so a term that cancels in the result still counts.

The row bound. For every row r along the last dimension of a bf16 output,

    ||got_r - want_r||_2 <= 2^-7 ||want_r||_2 + 2^-9 ||bud_r||_2

with the norms in float64. 2^-7 is two bf16 half-ulps (the output rounding,
plus the random-walk sum of the bf16 roundings of the P / dS operands, which
scales like the result); 2^-9 is one bf16 half-ulp of the uncancelled
magnitude (delta, and every term that cancels). Outputs that see only the
output rounding get the first term alone.

emulate_attn() is the calibration: attention in torch fp32 with the kernels'
bf16 roundings. The bound is right only if that honest implementation sits
well inside it; tests/test_kernel_check.py holds it to 0.5.
"""

import ctypes
import ctypes.util
import math

import torch

F64 = torch.float64
C_WANT = 2.0 ** -7      # two bf16 half-ulps of the result
C_BUD = 2.0 ** -9       # one bf16 half-ulp of the uncancelled magnitude
LSE_ATOL = 2.0 ** -12   # fp32 chain of a logsumexp, see docs/kernels.md


# ------------------------------------------------------------- the bounds
def _worst(ratio):
    ratio = torch.nan_to_num(ratio, nan=float("inf"), posinf=float("inf"))
    flat = ratio.reshape(-1)
    i = int(flat.argmax()) if flat.numel() else 0
    idx = tuple(int(j) for j in torch.unravel_index(torch.tensor(i),
                                                    ratio.shape)) \
        if ratio.dim() else ()
    return (float(flat[i]) if flat.numel() else 0.0), idx


def _ratio(err, bound):
    """err / bound with 0/0 = 0 and x/0 = inf; NaN in err stays NaN."""
    safe = torch.where(bound > 0, bound, torch.ones_like(bound))
    r = err / safe
    return torch.where(bound > 0, r,
                       torch.where(err == 0, torch.zeros_like(r),
                                   torch.full_like(r, float("inf"))))


def row_ratio(got, want, bud=None, c_want=C_WANT, c_bud=C_BUD):
    """Worst err / bound over the rows along the last dimension, and the
    index of that row. bud=None is the first term alone."""
    g, w = got.detach().cpu().to(F64), want.detach().cpu().to(F64)
    assert g.shape == w.shape, (g.shape, w.shape)
    err = (g - w).norm(dim=-1)
    bound = c_want * w.norm(dim=-1)
    if bud is not None:
        assert bud.shape == w.shape, (bud.shape, w.shape)
        bound = bound + c_bud * bud.cpu().to(F64).norm(dim=-1)
    return _worst(_ratio(err, bound))


def elem_ratio(got, want, bound):
    """Worst |got - want| / bound over the elements, and its index."""
    g, w = got.detach().cpu().to(F64), want.detach().cpu().to(F64)
    assert g.shape == w.shape, (g.shape, w.shape)
    return _worst(_ratio((g - w).abs(), bound.cpu().to(F64).expand_as(w)))


def assert_rows(got, want, bud=None, name="", limit=1.0, report=None):
    """The row bound as an assertion; the message names the worst row."""
    ratio, row = row_ratio(got, want, bud)
    if report is not None:
        report[name] = max(report.get(name, 0.0), ratio)
    print(f"[kernel_check] {name}: worst row {row} err/bound {ratio:.4f}")
    assert ratio <= limit, (
        f"{name}: row {row} is at {ratio:.3f} of its bound (limit {limit})")
    return ratio


def assert_elems(got, want, bound, name="", limit=1.0):
    ratio, idx = elem_ratio(got, want, bound)
    print(f"[kernel_check] {name}: worst element {idx} err/bound "
          f"{ratio:.4f}")
    assert ratio <= limit, (
        f"{name}: element {idx} is at {ratio:.3f} of its bound "
        f"(limit {limit})")
    return ratio


def assert_abs(got, want, atol, name=""):
    """|got - want| <= atol per element (fp32 outputs such as lse)."""
    g, w = got.detach().cpu().to(F64), want.detach().cpu().to(F64)
    return assert_elems(g, w, torch.full_like(w, atol), name)


def old_metric(got, want):
    """max|got - want| / max|want|: what the suite used alone before."""
    got, want = got.float(), want.float()
    return float((got - want).abs().max() / want.abs().max().clamp(min=1e-3))


def ulp32(x):
    """Spacing of fp32 at |x| (float64 tensor in, float64 out)."""
    a = x.abs().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


# -------------------------------------------------------------- attention
def visible(S, Skv, causal, doc_start=None, extra=None):
    """Boolean [B or 1, 1, S, Skv] of visible (q, kv) pairs, or None.
    Causal is bottom-right aligned (Skv >= S); doc_start[B,S] hides kv
    rows before the document's first; extra [S,Skv] is ANDed in (tests
    seed defects with it)."""
    mask = None
    if causal:
        mask = torch.ones(S, Skv, dtype=torch.bool).tril(
            diagonal=Skv - S).view(1, 1, S, Skv)
        if doc_start is not None:
            j = torch.arange(Skv).view(1, 1, 1, Skv)
            mask = mask & (j >= doc_start.long().cpu().view(-1, 1, S, 1))
    if extra is not None:
        e = extra.view(1, 1, S, Skv)
        mask = e if mask is None else mask & e
    return mask


def _bhsd(t, dtype):
    return t.detach().cpu().to(dtype).permute(0, 2, 1, 3)


def _bshd(t):
    return t.permute(0, 2, 1, 3).contiguous()


def _group_sum(t, B, Hkv, rep):
    return t.view(B, Hkv, rep, *t.shape[2:]).sum(dim=2) if rep > 1 else t


def attn_ref64(q, k, v, do=None, causal=True, scale=None, doc_start=None,
               extra=None):
    """fp64 attention from the bf16 inputs, BSHD like the ops. Returns a
    dict: o, lse [B,Hq,S] and bud_o; with do also dq, dk, dv and their
    budgets. The backward is the exact derivative: delta comes from the
    fp64 o, not from a rounded one."""
    B, S, Hq, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    rep = Hq // Hkv
    sc = 1.0 / math.sqrt(D) if scale is None else float(scale)
    qf, kf, vf = (_bhsd(t, F64) for t in (q, k, v))
    if rep > 1:
        kf = kf.repeat_interleave(rep, dim=1)
        vf = vf.repeat_interleave(rep, dim=1)
    s = qf @ kf.transpose(-1, -2) * sc
    mask = visible(S, Skv, causal, doc_start, extra)
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    del s
    o = p @ vf
    out = {"o": _bshd(o), "lse": lse, "bud_o": _bshd(p @ vf.abs())}
    if do is None:
        return out
    dof = _bhsd(do, F64)
    dv = p.transpose(-1, -2) @ dof
    bud_dv = p.transpose(-1, -2) @ dof.abs()
    dp = dof @ vf.transpose(-1, -2)
    delta = (dof * o).sum(dim=-1, keepdim=True)
    dbar = (dof.abs() * o.abs()).sum(dim=-1, keepdim=True)
    ds = p * (dp - delta) * sc
    wgt = p * (dp.abs() + dbar) * sc
    del dp, p
    out["dq"] = _bshd(ds @ kf)
    out["bud_dq"] = _bshd(wgt @ kf.abs())
    for name, t in (("dk", ds.transpose(-1, -2) @ qf),
                    ("bud_dk", wgt.transpose(-1, -2) @ qf.abs()),
                    ("dv", dv), ("bud_dv", bud_dv)):
        out[name] = _bshd(_group_sum(t, B, Hkv, rep))
    return out


def emulate_attn(q, k, v, do=None, causal=True, scale=None, doc_start=None):
    """The attention kernels' arithmetic in torch fp32 on the CPU: scores,
    exponentials and sums in fp32; P (unnormalised, exp(s - rowmax), in
    the forward; exp(s - lse) in the backward) and dS rounded to bf16
    before their matmuls; o rounded to bf16 and that o used for delta;
    outputs rounded to bf16."""
    f32, bf = torch.float32, torch.bfloat16
    B, S, Hq, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    rep = Hq // Hkv
    sc = 1.0 / math.sqrt(D) if scale is None else float(scale)
    qf, kf, vf = (_bhsd(t, f32) for t in (q, k, v))
    if rep > 1:
        kf = kf.repeat_interleave(rep, dim=1)
        vf = vf.repeat_interleave(rep, dim=1)
    s = qf @ kf.transpose(-1, -2) * sc
    mask = visible(S, Skv, causal, doc_start)
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    m = s.max(dim=-1, keepdim=True).values
    p = torch.exp(s - m)
    l = p.sum(dim=-1, keepdim=True)
    o = ((p.to(bf).to(f32) @ vf) / l).to(bf)
    lse = (m + torch.log(l)).squeeze(-1)
    out = {"o": _bshd(o), "lse": lse}
    if do is None:
        return out
    dof = _bhsd(do, f32)
    p = torch.exp(s - lse.unsqueeze(-1))
    pb = p.to(bf).to(f32)
    dv = pb.transpose(-1, -2) @ dof
    dp = dof @ vf.transpose(-1, -2)
    delta = (dof * o.to(f32)).sum(dim=-1, keepdim=True)
    ds = (p * (dp - delta) * sc).to(bf).to(f32)
    out["dq"] = _bshd((ds @ kf).to(bf))
    out["dk"] = _bshd(_group_sum(ds.transpose(-1, -2) @ qf, B, Hkv,
                                 rep).to(bf))
    out["dv"] = _bshd(_group_sum(dv, B, Hkv, rep).to(bf))
    return out


ATTN_OUTPUTS = ("o", "dq", "dk", "dv")

# (B, Hq, Hkv, S, Skv, D, causal). Forward edge shapes: less than one
# tile, one row into a second stage, a second kv block of one row, D=64
# ragged, GQA 4:1 with an odd stage count, non-causal with a kv tail,
# causal with Skv > S and both ragged.
ATTN_FWD_EDGE_CASES = [
    (1, 2, 2, 24, 24, 128, True),
    (1, 2, 2, 65, 65, 128, True),
    (1, 2, 2, 129, 129, 128, True),
    (2, 2, 2, 100, 100, 64, True),
    (1, 4, 1, 192, 192, 64, True),
    (1, 2, 2, 64, 200, 128, False),
    (1, 2, 2, 70, 197, 128, True),
]
# Shapes the backward runs at in the suite (S == Skv), the training shape
# last.
ATTN_BWD_CASES = [
    (1, 2, 2, 24, 24, 128, True),
    (1, 2, 2, 65, 65, 128, True),
    (1, 2, 2, 129, 129, 128, True),
    (1, 4, 1, 192, 192, 128, True),
    (2, 2, 2, 100, 100, 64, True),
    (1, 4, 1, 192, 192, 64, True),
    (1, 2, 2, 320, 320, 128, False),
    (1, 2, 2, 1024, 1024, 128, True),
]


def attn_inputs(B, Hq, Hkv, S, Skv, D, seed, scale=0.5):
    """CPU bf16 (q, k, v, do), N(0, scale^2) like the rest of the suite."""
    gen = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.randn(*s, generator=gen) * scale).to(
        torch.bfloat16)
    return mk(B, S, Hq, D), mk(B, Skv, Hkv, D), mk(B, Skv, Hkv, D), \
        mk(B, S, Hq, D)


def check_attn(got, want, names=ATTN_OUTPUTS, tag="", report=None,
               limit=1.0):
    """Row bound on the bf16 outputs in `names`, 2^-12 on lse if present
    in got. got / want are dicts as attn_ref64 returns them."""
    ratios = {}
    for n in names:
        ratios[n] = assert_rows(got[n], want[n], want["bud_" + n],
                                name=f"{tag}attn {n}", limit=limit,
                                report=report)
    if "lse" in got:
        ratios["lse"] = assert_abs(got["lse"], want["lse"], LSE_ATOL,
                                   name=f"{tag}attn lse")
    return ratios


# ---------------------------------------------------------------- rmsnorm
def rmsnorm_ref64(x, w, eps, dy=None, dres=None):
    """y, inv; with dy also dx, its budget, dw and the per-column sum
    bud_dw = sum_i |dy x inv|. x [M,H]."""
    xf, wf = x.detach().cpu().to(F64), w.detach().cpu().to(F64)
    H = xf.shape[-1]
    inv = torch.rsqrt(xf.pow(2).mean(dim=-1, keepdim=True) + eps)
    out = {"y": xf * inv * wf, "inv": inv.squeeze(-1)}
    if dy is None:
        return out
    dyf = dy.detach().cpu().to(F64)
    g = dyf * wf
    c = inv ** 3 / H * (g * xf).sum(dim=-1, keepdim=True)
    dx = inv * g - c * xf
    bud = (inv * g).abs() + (c * xf).abs()
    if dres is not None:
        dr = dres.detach().cpu().to(F64)
        dx = dx + dr
        bud = bud + dr.abs()
    t = dyf * xf * inv
    out.update(dx=dx, bud_dx=bud, dw=t.sum(dim=0), bud_dw=t.abs().sum(dim=0))
    return out


# ------------------------------------------------------------------- rope
def rope_ref64(x, cos, sin, pos, backward=False):
    """x [B,S,H,D]; pos [B,S] integer table rows. Returns (y, budget)
    with budget = |a cos| + |b sin| per element."""
    xf = x.detach().cpu().to(F64)
    D = xf.shape[-1]
    c = cos.detach().cpu().to(F64)[pos.long()].unsqueeze(2)   # [B,S,1,D/2]
    s = sin.detach().cpu().to(F64)[pos.long()].unsqueeze(2)
    if backward:
        s = -s
    x1, x2 = xf[..., :D // 2], xf[..., D // 2:]
    y = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    bud = torch.cat([(x1 * c).abs() + (x2 * s).abs(),
                     (x2 * c).abs() + (x1 * s).abs()], dim=-1)
    return y, bud


# ----------------------------------------------------------------- swiglu
def swiglu_ref64(g, u, d=None):
    gf, uf = g.detach().cpu().to(F64), u.detach().cpu().to(F64)
    sig = torch.sigmoid(gf)
    silu = gf * sig
    out = {"out": silu * uf}
    if d is None:
        return out
    df = d.detach().cpu().to(F64)
    out["dg"] = df * uf * (sig + silu * (1.0 - sig))
    out["bud_dg"] = (df * uf).abs() * (sig + silu.abs() * (1.0 - sig))
    out["du"] = df * silu
    return out


# ------------------------------------------------------------------- xent
def xent_ref64(logits, targets, dloss=None, ignore_index=-100):
    x = logits.detach().cpu().to(F64)
    t = targets.detach().cpu()
    lse = torch.logsumexp(x, dim=-1)
    live = t != ignore_index
    safe = t.masked_fill(~live, 0)
    picked = x.gather(-1, safe.unsqueeze(-1)).squeeze(-1)
    out = {"lse": lse,
           "loss": torch.where(live, lse - picked, torch.zeros_like(lse))}
    if dloss is not None:
        p = torch.exp(x - lse.unsqueeze(-1))
        p.scatter_add_(-1, safe.unsqueeze(-1), -torch.ones_like(p[:, :1]))
        out["dlogits"] = p * (dloss.detach().cpu().to(F64)
                              * live.to(F64)).unsqueeze(-1)
    return out


def xent_chunk_dlogits64(chunk, targets, lse, v0, ignore_index=-100):
    """exp(x - lse) - onehot for one vocabulary chunk starting at column
    v0, zero on ignored rows; lse is the full-row fp64 logsumexp."""
    x = chunk.detach().cpu().to(F64)
    t = targets.detach().cpu()
    dl = torch.exp(x - lse.unsqueeze(-1))
    inside = (t != ignore_index) & (t >= v0) & (t < v0 + x.shape[-1])
    rows = inside.nonzero(as_tuple=True)[0]
    dl[rows, t[rows] - v0] -= 1.0
    dl[t == ignore_index] = 0.0
    return dl


# ------------------------------------------------------------------ adamw
def _powf(base, exponent):
    """fp32 pow from the C library: the bias corrections are formed on the
    host in fp32, and 1 - beta2^step loses up to 1/(1 - beta2^step) of
    that rounding, so the reference takes the same fp32 value."""
    import numpy as np
    name = ctypes.util.find_library("m")
    if name:
        fn = ctypes.CDLL(name).powf
        fn.restype = ctypes.c_float
        fn.argtypes = [ctypes.c_float, ctypes.c_float]
        return float(fn(base, exponent))
    return float(np.float32(float(base) ** float(exponent)))


def adamw_ref64(master, grad, m, v, lr, beta1, beta2, eps, wd, step):
    """One AdamW step in fp64 from fp32 state. Every hyper-parameter is
    first rounded to the fp32 value the launcher hands the kernel,
    1 - beta, 1 - lr*wd and the inverse bias corrections included.
    Returns master, m, v, the step taken, and mag_m = |beta1 m| +
    |(1 - beta1) g|: the two terms of m have either sign, each product
    rounds at its own size, so ulps of m are counted at mag_m (v is a sum
    of non-negative terms and master is dominated by itself; where it is
    not, the step term of its bound is)."""
    import numpy as np
    f = np.float32
    lr, b1, b2, eps, wd = f(lr), f(beta1), f(beta2), f(eps), f(wd)
    one = f(1.0)
    inv_bc1 = float(one / (one - f(_powf(b1, f(step)))))
    inv_bc2 = float(one / (one - f(_powf(b2, f(step)))))
    omb1, omb2 = float(one - b1), float(one - b2)
    decay = float(one - lr * wd)
    g = grad.detach().cpu().to(F64)
    m0 = float(b1) * m.detach().cpu().to(F64)
    m2 = m0 + omb1 * g
    v2 = float(b2) * v.detach().cpu().to(F64) + omb2 * g * g
    denom = (v2 * inv_bc2).sqrt() + float(eps)
    took = float(lr) * inv_bc1 * m2 / denom
    p2 = master.detach().cpu().to(F64) * decay - took
    return {"master": p2, "m": m2, "v": v2, "took": took,
            "mag_m": m0.abs() + (omb1 * g).abs()}
