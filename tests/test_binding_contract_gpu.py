"""The binding contract (docs/kernels.md): per op, one valid call at the
smallest shape its kernel takes, compared with the reference under the
bound of the op's own GPU test, and the argument tuples the binding must
refuse.

Every refused input is memory-safe even for a binding without the check:
a wrong element count is larger than required, a strided argument is a
view into a larger buffer, a wrong dtype is no narrower, "not on the GPU"
is a pinned host tensor, and shapes the launchers fall through (D = 32)
launch nothing. One case is not built that way and only repeats a check
that was there before: `a` of gemm_nt with another inner dimension.

Refusals that cannot be built that way are not here: transpose_sd D % 64,
lora_wgrad K % 8, a rank-0 adapter in the contract kernels, dequant_int4
group <= 0, V = 0 logits, dropout_mask with a host `like` (each would
write or read past a buffer the binding itself sizes), and a first tensor
on another GPU than the current one (needs two devices).
"""

import math

import pytest
import torch

import kernel_check as kc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from datatunerx_amd import ops
    from datatunerx_amd.ops import _dtx_hip as hip
    from datatunerx_amd.ops import reference as ref
    DEV = torch.device("cuda:0")
    assert ops.have_ext(), "HIP extension must be built for GPU tests"

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
I32, I64 = torch.int32, torch.int64


def z(*shape, dt=BF):
    return torch.zeros(*shape, dtype=dt, device=DEV)


def rnd(*shape, dt=BF, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + 131 * len(shape) + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dt).to(DEV)


def pinned(*shape, dt=F32):
    """Host memory the device can address: refused, harmless if read."""
    return torch.zeros(*shape, dtype=dt).pin_memory()


def strided(n, dt=F32):
    """n elements, every other one of a buffer twice as long."""
    return z(2 * n, dt=dt)[::2]


def close(got, want, rtol=2e-2, name=""):
    """The metric of tests/test_ops_gpu.py."""
    got, want = got.float().cpu(), want.float().cpu()
    denom = want.abs().max().clamp(min=1e-3)
    err = (got - want).abs().max() / denom
    assert err < rtol, f"{name}: rel err {err:.4f} (max {denom:.3f})"


def refuse(fn, *args, match=None):
    with pytest.raises(RuntimeError, match=match):
        fn(*args)


def bad_kinds(n, dt, wide):
    """One argument of n elements of dtype dt, wrong in each way."""
    return [z(n, dt=wide), z(n + 8, dt=dt), strided(n, dt), pinned(n, dt=dt)]


# ---------------------------------------------------------------- row kernels
def test_rmsnorm_contract():
    x, w, dy = rnd(4, 64), rnd(64, seed=1), rnd(4, 64, seed=2)
    y, inv = hip.rmsnorm_fwd(x, w, 1e-5)
    y_r, inv_r = ref.rmsnorm_fwd(x.cpu(), w.cpu(), 1e-5)
    close(y, y_r, name="y")
    close(inv, inv_r, name="inv")
    dx, dw = hip.rmsnorm_bwd(dy, x, w, inv, None)
    dx_r, dw_r = ref.rmsnorm_bwd(dy.cpu(), x.cpu(), w.cpu(), inv_r)
    close(dx, dx_r, name="dx")
    close(dw, dw_r, rtol=3e-2, name="dw")
    refuse(hip.rmsnorm_fwd, x, pinned(64, dt=BF), 1e-5, match="w must")
    refuse(hip.rmsnorm_bwd, dy, x, w, pinned(4), None, match="inv")
    refuse(hip.rmsnorm_bwd, dy, x, w, inv, pinned(4, 64, dt=BF),
           match="dres")
    # empty work: shaped outputs, a zero dw, no launch
    y0, inv0 = hip.rmsnorm_fwd(z(0, 64), w, 1e-5)
    assert y0.shape == (0, 64) and inv0.shape == (0,)
    dx0, dw0 = hip.rmsnorm_bwd(z(0, 64), z(0, 64), w, z(0, dt=F32), None)
    assert dx0.shape == (0, 64) and torch.equal(dw0, z(64, dt=F32))
    torch.cuda.synchronize()


def test_swiglu_contract():
    g, u, d = rnd(4, 64), rnd(4, 64, seed=1), rnd(4, 64, seed=2)
    close(hip.swiglu_fwd(g, u), ref.swiglu_fwd(g.cpu(), u.cpu()), name="out")
    dg, du = hip.swiglu_bwd(d, g, u)
    dg_r, du_r = ref.swiglu_bwd(d.cpu(), g.cpu(), u.cpu())
    close(dg, dg_r, name="dg")
    close(du, du_r, name="du")
    refuse(hip.swiglu_fwd, g, z(4, 128), match="up")            # up shape
    refuse(hip.swiglu_fwd, g, z(4, 128)[:, ::2], match="up")    # up strided
    refuse(hip.swiglu_fwd, g, pinned(4, 64, dt=BF), match="up")
    assert hip.swiglu_fwd(z(0, 64), z(0, 64)).shape == (0, 64)
    torch.cuda.synchronize()


def test_rope_contract():
    B, S, H, D = 1, 4, 2, 8
    x = rnd(B, S, H, D)
    # the tables are rows 1..8 of a 10-row buffer: row -1 is still inside
    cos_t, sin_t = ref.rope_tables(10, D)
    cos, sin = cos_t.to(DEV)[1:9], sin_t.to(DEV)[1:9]
    assert cos.is_contiguous() and cos.shape == (8, D // 2)
    for bwd, fn in ((False, ref.rope_fwd), (True, ref.rope_bwd)):
        y = hip.rope(x, cos, sin, 2, bwd, None, None)
        close(y, fn(x.cpu(), cos.cpu(), sin.cpu(), 2), name=f"rope {bwd}")
    # pos_dev of one element and of B elements
    x2 = rnd(2, S, H, D, seed=3)
    for pos in ([3], [0, 4]):
        pd = torch.tensor(pos, dtype=I32)
        y = hip.rope(x2, cos, sin, 0, False, pd.to(DEV), None)
        want = ops.rope_fwd(x2.cpu(), cos.cpu(), sin.cpu(), 0, pd)
        close(y, want, name=f"rope pos_dev {pos}")
    pd = z(2, dt=I32)
    for args in [
        (x, z(8, 4, dt=F64), sin, 0, False, None, None),        # cosb dtype
        (x, z(8, 8, dt=F32), z(8, 8, dt=F32), 0, False, None, None),  # width
        (x, z(32, dt=F32), z(32, dt=F32), 0, False, None, None),  # not 2-D
        (x, z(8, 8, dt=F32)[:, ::2], sin, 0, False, None, None),  # strided
        (x, pinned(8, 4), sin, 0, False, None, None),           # on the host
    ]:
        refuse(hip.rope, *args, match="cosb")
    for bad_sin in (z(8, 4, dt=F64), z(9, 4, dt=F32), z(8, 8, dt=F32)[:, ::2],
                    pinned(8, 4)):
        refuse(hip.rope, x, cos, bad_sin, 0, False, None, None, match="sinb")
    refuse(hip.rope, x, cos, sin, -1, False, None, None, match="pos0")
    for bad_pd in (z(2, dt=I64), z(3, dt=I32), strided(2, I32),
                   pinned(2, dt=I32)):
        refuse(hip.rope, x2, cos, sin, 0, False, bad_pd, None,
               match="pos_dev")
    assert hip.rope(z(0, S, H, D), cos, sin, 0, False, None, None).shape == \
        (0, S, H, D)
    assert hip.rope(x2, cos, sin, 0, False, pd, None).shape == x2.shape
    torch.cuda.synchronize()


# ------------------------------------------------------------ cross entropy
def test_xent_contract():
    N, V = 4, 64
    logits = rnd(N, V, scale=3.0)
    targets = torch.tensor([0, V - 1, -100, 5], device=DEV)
    dloss = torch.rand(N, generator=torch.Generator().manual_seed(1)).to(DEV)
    loss, lse = hip.xent_fwd(logits, targets, -100)
    loss_r, lse_r = ref.softmax_xent_fwd(logits.cpu(), targets.cpu())
    close(loss, loss_r, rtol=1e-2, name="loss")
    close(lse, lse_r, rtol=1e-2, name="lse")
    dl = hip.xent_bwd(logits, targets, lse, dloss, -100)
    close(dl, ref.softmax_xent_bwd(logits.cpu(), targets.cpu(), lse_r,
                                   dloss.cpu()), rtol=3e-2, name="dlogits")
    # the chunk kernels: this chunk is columns 32..95 of a wider vocabulary
    v0 = 32
    tg = torch.tensor([32, 95, -100, 200], device=DEV)
    m, l, t = torch.full((N,), -3.4e38, device=DEV), z(N, dt=F32), z(N, dt=F32)
    hip.xent_lse_merge(logits, tg, m, l, t, v0, -100)
    m_r, l_r, t_r = torch.full((N,), -3.4e38), torch.zeros(N), torch.zeros(N)
    ref.xent_lse_merge(logits.cpu(), tg.cpu(), m_r, l_r, t_r, v0)
    for got, want, name in ((m, m_r, "m"), (l, l_r, "l"), (t, t_r, "tgt")):
        close(got, want, name=f"chunk {name}")
    lse_c = m + l.log()
    close(hip.xent_dlogits(logits, tg, lse_c, v0, -100),
          ref.xent_dlogits(logits.cpu(), tg.cpu(), lse_c.cpu(), v0),
          name="chunk dlogits")

    f = lambda n=N: z(n, dt=F32)
    calls = {      # op -> (call with logits, targets and the f32 vectors)
        "fwd": lambda lg, tt, a, b, c: hip.xent_fwd(lg, tt, -100),
        "bwd": lambda lg, tt, a, b, c: hip.xent_bwd(lg, tt, a, b, -100),
        "merge": lambda lg, tt, a, b, c: hip.xent_lse_merge(lg, tt, a, b, c,
                                                            0, -100),
        "dlogits": lambda lg, tt, a, b, c: hip.xent_dlogits(lg, tt, a, 0,
                                                            -100),
    }
    zt = z(N, dt=I64)
    for name, call in calls.items():
        refuse(call, z(N, 60), zt, f(), f(), f(), match="V % 8")
        for bad_t in bad_kinds(N, I64, F64):
            refuse(call, logits, bad_t, f(), f(), f(), match="targets")
    for bad in bad_kinds(N, F32, F64):
        refuse(calls["bwd"], logits, zt, bad, f(), f(), match="lse")
        refuse(calls["bwd"], logits, zt, f(), bad, f(), match="dloss")
        refuse(calls["merge"], logits, zt, bad, f(), f(), match="m_run")
        refuse(calls["merge"], logits, zt, f(), bad, f(), match="l_run")
        refuse(calls["merge"], logits, zt, f(), f(), bad, match="tgt")
        refuse(calls["dlogits"], logits, zt, bad, f(), f(), match="lse")
    refuse(hip.xent_lse_merge, logits, zt, f(), f(), f(), -1, -100,
           match="v0")
    refuse(hip.xent_dlogits, logits, zt, f(), -1, -100, match="v0")
    # empty work: N = 0 used to be a launch with an empty grid
    e, et = z(0, V), z(0, dt=I64)
    assert [x.shape for x in hip.xent_fwd(e, et, -100)] == [(0,), (0,)]
    assert hip.xent_bwd(e, et, f(0), f(0), -100).shape == (0, V)
    hip.xent_lse_merge(e, et, f(0), f(0), f(0), 0, -100)
    assert hip.xent_dlogits(e, et, f(0), 0, -100).shape == (0, V)
    torch.cuda.synchronize()


# -------------------------------------------------------------------- adamw
def test_adamw_contract():
    n = 8
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.01)
    master, g = rnd(n, dt=F32), rnd(n, dt=F32, seed=1)
    p, m, v = master.to(BF), z(n, dt=F32), z(n, dt=F32)
    cpu = [t.cpu().clone() for t in (p, master, g, m, v)]
    for step in (1, 2):
        before = tuple(t.cpu().clone() for t in (master, m, v))
        hip.adamw(p, master, g, m, v, *hp, step)
        ref.adamw_step(*cpu, *hp, step)
        # v and p under the bounds of test_adamw_bounds, against the fp64
        # reference that rounds 1 - beta2 to fp32 as the kernel does
        # (ops/reference.py forms it in double: up to 2^-24 / 0.001 = 6e-5
        # of v apart, so v has no bound against that one)
        want = kc.adamw_ref64(before[0], g.cpu(), before[1], before[2], *hp,
                              step)
        kc.assert_elems(v, want["v"], 4 * kc.ulp32(want["v"]),
                        name=f"adamw v @{step}")
        assert torch.equal(p, master.to(BF)), f"adamw p @{step}"
    close(master, cpu[1], rtol=1e-5, name="master")
    close(m, cpu[3], rtol=1e-5, name="m")
    ok = lambda: [z(n), z(n, dt=F32), z(n, dt=F32), z(n, dt=F32),
                  z(n, dt=F32)]
    for i, name in ((1, "master"), (2, "grad"), (3, "m"), (4, "v")):
        for bad in bad_kinds(n, F32, F64):
            args = ok()
            args[i] = bad
            refuse(hip.adamw, *args, *hp, 1, match=name + " must")
    refuse(hip.adamw, *ok(), *hp, 0, match="step")
    hip.adamw(z(0), *[z(0, dt=F32) for _ in range(4)], *hp, 1)   # empty
    torch.cuda.synchronize()


# ---------------------------------------------------------------- attention
def _attn(B=1, S=8, Skv=8, Hq=2, Hkv=1, D=64):
    return (rnd(B, S, Hq, D, scale=0.5),
            rnd(B, Skv, Hkv, D, scale=0.5, seed=1),
            rnd(B, Skv, Hkv, D, scale=0.5, seed=2))


def test_attn_fwd_bwd_contract():
    B, S, Hq, D = 1, 8, 2, 64
    sc = 1.0 / math.sqrt(D)
    q, k, v = _attn()
    o, lse = hip.attn_fwd(q, k, v, True, sc)
    o_r, lse_r = ref.attn_fwd(q.cpu(), k.cpu(), v.cpu(), True)
    close(o, o_r, name="o")
    close(lse, lse_r, rtol=1e-2, name="lse")
    # dO as autograd may hand it over: a permuted, non-contiguous view
    dO = rnd(B, Hq, S, D, seed=3).permute(0, 2, 1, 3)
    assert not dO.is_contiguous()
    grads = hip.attn_bwd(q, k, v, o, dO, lse, True, sc)
    want = ref.attn_bwd(q.cpu(), k.cpu(), v.cpu(), o_r, dO.cpu(), lse_r, True)
    for got, w, name in zip(grads, want, ("dq", "dk", "dv")):
        close(got, w, rtol=3e-2, name=name)
    for got, w in zip(grads, hip.attn_bwd(q, k, v, o, dO.contiguous(), lse,
                                          True, sc)):
        assert torch.equal(got, w)

    def both(qq, kk, vv, match):
        refuse(hip.attn_fwd, qq, kk, vv, True, sc, match=match)
        refuse(hip.attn_bwd, qq, kk, vv, z(*qq.shape), z(*qq.shape),
               z(1, 2, 8, dt=F32), True, sc, match=match)

    both(z(8, 2, 64), k, v, "q must")                       # q not 4-D
    both(q, z(2, 8, 1, 64), z(2, 8, 1, 64), "k must")       # k batch
    both(q, z(8, 1, 64), v, "k must")                       # k not 4-D
    both(q, k, z(1, 16, 1, 64), "v must")                   # v shape
    both(q, k, pinned(1, 8, 1, 64, dt=BF), "v must")
    both(z(1, 0, 2, 64), k, v, "S >= 1")
    both(q, z(1, 0, 1, 64), z(1, 0, 1, 64), "Skv >= 1")
    # Hq = 3 over Hkv = 2: head index 2 stays inside a batch-2 buffer
    both(z(1, 8, 3, 64), z(2, 8, 2, 64)[:1], z(2, 8, 2, 64)[:1], "Hq % Hkv")
    q32 = z(1, 8, 2, 32)                  # D = 32: the launchers run nothing
    both(q32, z(1, 8, 1, 32), z(1, 8, 1, 32), "D must")
    bwd = lambda o_, dO_, lse_: (q, k, v, o_, dO_, lse_, True, sc)
    dOc = dO.contiguous()
    refuse(hip.attn_bwd, *bwd(z(1, 16, 2, 64), dOc, lse), match="o must")
    refuse(hip.attn_bwd, *bwd(pinned(1, 8, 2, 64, dt=BF), dOc, lse),
           match="o must")
    refuse(hip.attn_bwd, *bwd(o, z(1, 8, 2, 64, dt=F32), lse), match="dO")
    refuse(hip.attn_bwd, *bwd(o, z(1, 16, 2, 64), lse), match="dO")
    refuse(hip.attn_bwd, *bwd(o, pinned(1, 8, 2, 64, dt=BF), lse), match="dO")
    for bad in (z(1, 2, 8, dt=F64), z(1, 2, 16, dt=F32),
                z(1, 2, 16, dt=F32)[:, :, ::2], pinned(1, 2, 8),
                z(16, dt=F32)):
        refuse(hip.attn_bwd, *bwd(o, dOc, bad), match="lse")
    # empty batch
    e = [z(0, 8, 2, 64), z(0, 8, 1, 64), z(0, 8, 1, 64)]
    o0, lse0 = hip.attn_fwd(*e, True, sc)
    assert o0.shape == (0, 8, 2, 64) and lse0.shape == (0, 2, 8)
    g0 = hip.attn_bwd(*e, o0, o0, lse0, True, sc)
    assert [t.shape for t in g0] == [t.shape for t in e]
    torch.cuda.synchronize()


def test_attn_decode_contract():
    Hq, Hkv, D, n = 2, 1, 64, 8
    sc = 1.0 / math.sqrt(D)
    # B = 1: the prefix view of a larger cache, as the serving engine has it
    q = rnd(1, 1, Hq, D, scale=0.5)
    kc_, vc_ = rnd(1, 32, Hkv, D, scale=0.5, seed=1), \
        rnd(1, 32, Hkv, D, scale=0.5, seed=2)
    k, v = kc_[:, :n], vc_[:, :n]
    o_r, lse_r = ref.attn_fwd(q.cpu(), k.cpu(), v.cpu(), True)
    ld = torch.tensor([n], dtype=I32, device=DEV)      # len_dev of one
    for kk, vv, ll in ((k, v, None), (k, v, ld), (kc_, vc_, ld)):
        o, lse = hip.attn_decode(q, kk, vv, sc, ll)
        close(o, o_r, name="decode o")
        close(lse.reshape(-1), lse_r.reshape(-1), rtol=1e-2, name="lse")
    # len_dev of B elements
    q2 = rnd(2, 1, Hq, D, scale=0.5, seed=3)
    k2, v2 = rnd(2, n, Hkv, D, scale=0.5, seed=4), \
        rnd(2, n, Hkv, D, scale=0.5, seed=5)
    lens = [n, 5]
    o, lse = hip.attn_decode(q2, k2, v2, sc,
                             torch.tensor(lens, dtype=I32, device=DEV))
    for b, nb in enumerate(lens):
        o_b, lse_b = ref.attn_fwd(q2[b:b + 1].cpu(), k2[b:b + 1, :nb].cpu(),
                                  v2[b:b + 1, :nb].cpu(), True)
        close(o[b:b + 1], o_b, name=f"decode row {b}")
        close(lse[b].reshape(-1), lse_b.reshape(-1), rtol=1e-2, name="lse")

    refuse(hip.attn_decode, q, k, z(1, 16, Hkv, D), sc, None, match="v must")
    refuse(hip.attn_decode, q, z(2, n, Hkv, D), z(2, n, Hkv, D), sc, None,
           match="k must")
    refuse(hip.attn_decode, q, z(n, Hkv, D), v, sc, None, match="k must")
    refuse(hip.attn_decode, q, z(1, n, Hkv, 128), z(1, n, Hkv, 128), sc, None,
           match="k must")                                  # k, v of D = 128
    refuse(hip.attn_decode, q, z(1, n, Hkv, D, dt=F32), v, sc, None,
           match="k must")
    refuse(hip.attn_decode, q, pinned(1, n, Hkv, D, dt=BF), v, sc, None,
           match="k must")
    refuse(hip.attn_decode, q, z(1, 0, Hkv, D), z(1, 0, Hkv, D), sc, None,
           match="Skv >= 1")
    # Hq = 3 over Hkv = 2, on views of a longer cache (a head index one
    # past Hkv stays inside it)
    big = z(1, 32, 2, D)
    refuse(hip.attn_decode, z(1, 1, 3, D), big[:, :n], big[:, :n], sc, None,
           match="Hq % Hkv")
    for bad in (z(2, dt=I64), z(3, dt=I32), strided(2, I32),
                pinned(2, dt=I32)):
        refuse(hip.attn_decode, q2, k2, v2, sc, bad, match="len_dev")
    o0, lse0 = hip.attn_decode(z(0, 1, Hq, D), z(0, n, Hkv, D),
                               z(0, n, Hkv, D), sc, None)
    assert o0.shape == (0, 1, Hq, D) and lse0.shape == (0, Hq, 1)
    torch.cuda.synchronize()


def test_transpose_sd_contract():
    x = rnd(1, 8, 2, 64)
    assert torch.equal(hip.transpose_sd(x), x.permute(0, 2, 3, 1).contiguous())
    refuse(hip.transpose_sd, z(8, 2, 64), match="x must")
    refuse(hip.transpose_sd, z(1, 8, 2, 128)[..., ::2], match="x must")
    assert hip.transpose_sd(z(0, 8, 2, 64)).shape == (0, 2, 64, 8)
    torch.cuda.synchronize()


# ------------------------------------------------------- GEMM, GEMV, dequant
def test_gemm_gemv_contract():
    a, b, src = rnd(8, 128), rnd(256, 128, seed=1), rnd(8, 256, seed=2)
    close(hip.gemm_nt(a, b, None), a.float() @ b.float().t(), name="gemm_nt")
    close(hip.gemm_nt(a, b, src), a.float() @ b.float().t() + src.float(),
          name="gemm_nt+src")
    refuse(hip.gemm_nt, a, z(1, 256, 128), None, match="b must")
    refuse(hip.gemm_nt, z(8, 256), b, None, match="a must")   # an old check
    refuse(hip.gemm_nt, a, b, z(16, 256), match="src")
    assert hip.gemm_nt(z(0, 128), b, None).shape == (0, 256)

    x, w = rnd(1, 64, scale=0.3), rnd(8, 64, scale=0.3, seed=1)
    close(hip.gemv(x, w), torch.nn.functional.linear(x.float(), w.float()),
          name="gemv")
    refuse(hip.gemv, x, z(1, 8, 64), match="w must")
    refuse(hip.gemv, z(1, 2, 32), w, match="x must")       # 64 elements
    refuse(hip.gemv, x, pinned(8, 64, dt=BF), match="w must")
    torch.cuda.synchronize()


def test_dequant_contract():
    from datatunerx_amd.models.quant import (dequantize_int4,
                                             dequantize_int8, quantize_int4,
                                             quantize_int8)
    N, K = 8, 64
    w = rnd(N, K).cpu()
    q8, s8 = quantize_int8(w)
    close(hip.dequant_int8(q8.to(DEV), s8.to(DEV)),
          dequantize_int8(q8, s8, torch.float32), name="int8")
    q4, s4 = quantize_int4(w)
    close(hip.dequant_int4(q4.to(DEV), s4.to(DEV), 64),
          dequantize_int4(q4, s4, torch.float32), name="int4")
    q8d, q4d = q8.to(DEV), q4.to(DEV)
    refuse(hip.dequant_int8, q8d.view(1, N, K), s8.to(DEV), match="q must")
    refuse(hip.dequant_int4, q4d.view(1, N, K // 2), s4.to(DEV), 64,
           match="packed must")
    for bad in bad_kinds(N, F32, F64):
        refuse(hip.dequant_int8, q8d, bad, match="scale")
        refuse(hip.dequant_int4, q4d, bad, 64, match="scale")
    # K % group: 64 % 48; the scales are sized for the smaller group of 8
    refuse(hip.dequant_int4, q4d, z(N * 8, dt=F32), 48, match="K % group")
    assert hip.dequant_int8(z(0, K, dt=torch.int8), z(0, dt=F32)).shape == \
        (0, K)
    torch.cuda.synchronize()


# --------------------------------------------------------------------- LoRA
def test_lora_contract():
    M, K, N, r = 8, 64, 64, 8
    x = rnd(M, K, scale=0.3)
    w0, w1 = rnd(r, K, scale=0.3, seed=1), rnd(r, K, scale=0.3, seed=2)
    mask = ops.dropout_mask(M, K, 7, 0.9, x)
    assert torch.equal(mask.cpu(), ref.dropout_mask(M, K, 7, 0.9))
    # contract with and without a mask; the dual form
    close(hip.lora_contract(x, w0), ref.lora_contract(x.cpu(), w0.cpu()),
          name="contract")
    close(hip.lora_contract(x, w0, mask),
          ref.lora_contract(x.cpu(), w0.cpu(), mask.cpu()), name="masked")
    for got, w in zip(hip.lora_contract2(x, w0, w1), (w0, w1)):
        assert torch.equal(got, hip.lora_contract(x, w))
    t0, t1 = rnd(M, r, dt=F32, seed=3), rnd(M, r, dt=F32, seed=4)
    y = rnd(M, N, seed=5)
    y1 = y.clone()
    hip.lora_expand_add_t(y1, t0, w0, 0.5)
    close(y1, ref.lora_expand_add_t(y.cpu().clone(), t0.cpu(), w0.cpu(), 0.5),
          name="expand_add_t")
    y2 = y.clone()
    hip.lora_expand_add2(y2, t0, t1, w0, w1, 0.5)
    close(y2, ref.lora_expand_add2(y.cpu().clone(), t0.cpu(), t1.cpu(),
                                   w0.cpu(), w1.cpu(), 0.5), name="expand2")
    close(hip.lora_wgrad(t0, x, 0.7), ref.lora_wgrad(t0.cpu(), x.cpu(), 0.7),
          name="wgrad")

    zt = lambda: z(M, r, dt=F32)
    refuse(hip.lora_contract, x, z(1, r, K), match="w must")     # w not 2-D
    refuse(hip.lora_contract, x, w0, pinned(M, K, dt=BF), match="mask")
    refuse(hip.lora_contract, x, w0, z(2 * M, K), match="mask")
    refuse(hip.lora_contract, x, w0, None, 0, 0.0, match="keep")
    refuse(hip.lora_contract2, x, w0, z(2 * r, K), match="w1")
    refuse(hip.lora_contract2, x, w0, w1, 0, 0, 1.5, match="keep")
    yz = z(M, N)
    for bad in (z(M * r, dt=F64), z(M + 1, r, dt=F32), strided(M * r),
                pinned(M, r)):
        refuse(hip.lora_expand_add_t, yz, bad, w0, 0.5, match="t must")
        refuse(hip.lora_expand_add2, yz, bad, zt(), w0, w1, 0.5,
               match="t0 must")
        refuse(hip.lora_expand_add2, yz, zt(), bad, w0, w1, 0.5,
               match="t1 must")
        refuse(hip.lora_wgrad, bad, x, 0.5, match="t must")
    refuse(hip.lora_expand_add_t, yz, z(M, 0, dt=F32), z(0, N), 0.5,
           match="wt must")                                      # r = 0
    refuse(hip.lora_expand_add_t, yz, zt(), z(1, r, N), 0.5, match="wt must")
    refuse(hip.lora_expand_add_t, yz, zt(), w0, 0.5, None, 0, 0.0,
           match="keep")
    # N % 8: rows of 60 in buffers twice as long
    refuse(hip.lora_expand_add_t, z(2 * M, 60)[:M], zt(), z(2 * r, 60)[:r],
           0.5, match="% 8")
    refuse(hip.lora_expand_add2, yz, zt(), zt(), w0, z(2 * r, N), 0.5,
           match="a1")
    refuse(hip.lora_expand_add2, yz, zt(), zt(), w0, w1, 0.5, 0, 0, 0.0,
           match="keep")
    refuse(hip.lora_wgrad, zt(), x, 0.5, pinned(M, K, dt=BF), match="mask")
    refuse(hip.lora_wgrad, zt(), x, 0.5, None, 0, 0.0, match="keep")
    refuse(hip.dropout_mask, M, K, 7, 0.0, x, match="keep")
    # empty work: shaped outputs, a zero gradient, no launch
    assert hip.lora_contract(z(0, K), w0).shape == (0, r)
    assert [t.shape for t in hip.lora_contract2(z(0, K), w0, w1)] == \
        [(0, r), (0, r)]
    hip.lora_expand_add_t(z(0, N), z(0, r, dt=F32), w0, 0.5)
    hip.lora_expand_add2(z(0, N), z(0, r, dt=F32), z(0, r, dt=F32), w0, w1,
                         0.5)
    assert torch.equal(hip.lora_wgrad(z(0, r, dt=F32), z(0, K), 0.5),
                       z(r, K, dt=F32))
    assert hip.dropout_mask(0, K, 7, 0.9, x).shape == (0, K)
    torch.cuda.synchronize()


# ------------------------------------------------ already complete: edge forms
def test_sample_on_row_strided_view():
    """logits[:, -1] of a [B, S, V] tensor: dense rows, strided batch."""
    B, V = 2, 64
    full = rnd(B, 3, V, scale=3.0)
    last = full[:, -1]
    assert not last.is_contiguous()
    par = (z(B, dt=F32), torch.ones(B, device=DEV), z(B, dt=I32),
           z(B, dt=I64), z(B, dt=I32))               # temperature 0: greedy
    got = hip.sample(last, *par)
    assert torch.equal(got, hip.sample(last.contiguous(), *par))
    assert torch.equal(got.cpu(), ref.sample(last.cpu(), *[p.cpu()
                                                           for p in par]))
    refuse(hip.sample, full[:, -1, ::2], *par, match="logits")
    refuse(hip.sample, last, pinned(B), *par[1:], match="temperature")
    torch.cuda.synchronize()
