"""HIP kernels against fp64 references under the row-wise bounds of
tests/kernel_check.py (docs/kernels.md, "Numerics bounds"), at the entry
modes and loop paths that had no reference comparison on the GPU:
rmsnorm_bwd with dres, the row grid-stride loops, rope with pos_dev,
attn_decode with len_dev, the forward attention edge shapes, the xent
chunk kernels with a moving maximum, and AdamW's v / bf16 outputs.
"""

import math
import zlib

import pytest
import torch

import kernel_check as kc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from datatunerx_amd import ops
    from datatunerx_amd.ops import _dtx_hip
    DEV = torch.device("cuda:0")
    assert ops.have_ext(), "HIP extension must be built for GPU tests"

BF = torch.bfloat16


def gen_of(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


# ---------------------------------------------------------------- rmsnorm
# (4100, 64): forward grid-stride (grid 4096). (1030, 64): backward
# grid-stride (grid 1024). (3, 8): one group, 255 idle threads.
# (5, 2056): 257 groups, thread 0 owns two. (2, 16384): the widest row.
@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("M,H", [(4100, 64), (1030, 64), (3, 8), (5, 2056),
                                 (2, 16384)])
def test_rmsnorm_bounds(M, H, with_dres):
    g = gen_of("rmsnorm", M, H)
    # row magnitudes over four decades: a row-wise bound sees every row
    rows = torch.pow(10.0, torch.rand(M, 1, generator=g) * 4 - 2)
    x = (randn(g, M, H) * rows).to(BF)
    w = (1.0 + 0.5 * randn(g, H)).to(BF)
    dy = randn(g, M, H).to(BF)
    dres = randn(g, M, H).to(BF) if with_dres else None
    eps = 1e-5
    want = kc.rmsnorm_ref64(x, w, float(torch.tensor(eps).float()), dy, dres)

    y, inv = ops.rmsnorm_fwd(x.to(DEV), w.to(DEV), eps)
    kc.assert_rows(y, want["y"], name="rmsnorm y")
    kc.assert_elems(inv, want["inv"], 2.0 ** -20 * want["inv"].abs(),
                    name="rmsnorm inv")
    dx, dw = ops.rmsnorm_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), inv,
                             dres.to(DEV) if with_dres else None)
    kc.assert_rows(dx, want["dx"], want["bud_dx"], name="rmsnorm dx")
    # one fp32 rounding per added row, M * 2^-24 <= 2^-12 at M <= 4100
    kc.assert_elems(dw, want["dw"], 2.0 ** -12 * want["bud_dw"],
                    name="rmsnorm dw")


def test_rmsnorm_and_swiglu_bindings_refuse_bad_input():
    """The checks fire before any launch: nothing runs on the device.
    H = 16392 used to drop the columns past 16384 without a word."""
    z = lambda *s, dt=BF: torch.zeros(*s, dtype=dt, device=DEV)
    with pytest.raises(RuntimeError, match="16384"):
        _dtx_hip.rmsnorm_fwd(z(2, 16392), z(16392), 1e-5)
    with pytest.raises(RuntimeError, match="16384"):
        _dtx_hip.rmsnorm_bwd(z(2, 16392), z(2, 16392), z(16392),
                             z(2, dt=torch.float32), None)
    x, w, inv = z(4, 64), z(64), z(4, dt=torch.float32)
    bad = [
        (z(4, 60), z(4, 60), z(60), inv, None),            # H % 8
        (x, x, z(64, dt=torch.float32), inv, None),        # w not bf16
        (x, x, z(128)[::2], inv, None),                    # w strided
        (x, x, z(32), inv, None),                          # w length
        (x, x, w, z(4, dt=torch.float64), None),           # inv not fp32
        (x, x, w, z(3, dt=torch.float32), None),           # inv length
        (z(2, 128), x, w, inv, None),                      # dy shape
        (x, x, w, inv, z(4, 32)),                          # dres shape
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            _dtx_hip.rmsnorm_bwd(*args)
    with pytest.raises(RuntimeError):
        _dtx_hip.rmsnorm_fwd(x, z(32), 1e-5)               # w length
    g = z(4, 64)
    for args in [(g, z(4, 64, dt=torch.float32), g),       # gate dtype
                 (g, g, z(4, 128)[:, ::2]),                # up strided
                 (g, z(4, 32), g),                         # gate shape
                 (g, g, z(4, 32)),                         # up shape
                 (z(3, 4), z(3, 4), z(3, 4))]:             # numel % 8
        with pytest.raises(RuntimeError):
            _dtx_hip.swiglu_bwd(*args)


# ------------------------------------------------------------------- rope
TABLE = 64


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("mode", ["pos0", "pos_dev_scalar", "pos_dev_rows"])
@pytest.mark.parametrize("D", [64, 128])
def test_rope_bounds(D, mode, backward):
    B, S, H = 3, 5, 2
    g = gen_of("rope", D)
    x = randn(g, B, S, H, D).to(BF)
    cos, sin = ops.rope_tables(TABLE, D)
    s = torch.arange(S).view(1, S)
    if mode == "pos0":
        pos0, pos_dev, pos = 7, None, (7 + s).expand(B, S)
    elif mode == "pos_dev_scalar":
        pos0, pos_dev = 2, torch.tensor([9], dtype=torch.int32)
        pos = (11 + s).expand(B, S)
    else:
        pos0 = 0
        pos_dev = torch.tensor([0, 11, TABLE - S], dtype=torch.int32)
        pos = pos_dev.long().view(B, 1) + s
    assert int(pos.max()) < TABLE
    want, bud = kc.rope_ref64(x, cos, sin, pos, backward)
    got = _dtx_hip.rope(x.to(DEV), cos.to(DEV), sin.to(DEV), pos0, backward,
                        pos_dev.to(DEV) if pos_dev is not None else None,
                        None)
    kc.assert_elems(got, want, 2.0 ** -8 * bud, name=f"rope {mode}")
    if not backward:     # the public wrapper takes the same route
        y = ops.rope_fwd(x.to(DEV), cos.to(DEV), sin.to(DEV), pos0,
                         pos_dev.to(DEV) if pos_dev is not None else None)
        assert torch.equal(y, got)


# ----------------------------------------------------------------- swiglu
SWIGLU_FLOOR = 1e-30    # g = -88 gives ~5e-37, where v_rcp_f32 may flush
GATES = [0.0, -0.0, 1.278, -1.278, 20.0, -20.0, 88.0, -88.0, -89.0, -100.0,
         1e4]


def _swiglu_check(g, u, d):
    want = kc.swiglu_ref64(g, u, d)
    out = ops.swiglu_fwd(g.to(DEV), u.to(DEV))
    dg, du = ops.swiglu_bwd(d.to(DEV), g.to(DEV), u.to(DEV))
    for name, t in (("out", out), ("dg", dg), ("du", du)):
        assert bool(torch.isfinite(t.float()).all()), f"swiglu {name}"
        bound = kc.C_WANT * want[name].abs() + SWIGLU_FLOOR
        if name == "dg":
            bound = bound + kc.C_BUD * want["bud_dg"]
        kc.assert_elems(t, want[name], bound, name=f"swiglu {name}")


def test_swiglu_bounds_random():
    g = gen_of("swiglu")
    shape = (1030, 520)                 # 66950 groups of 8: a ragged grid
    _swiglu_check((randn(g, *shape) * 3).to(BF), randn(g, *shape).to(BF),
                  randn(g, *shape).to(BF))


def test_swiglu_bounds_fixed_gates():
    """Signed zero, the minimum of silu', saturation on both sides, the
    gates where exp(-g) overflows fp32 (-89, -100) or 1/(1+exp(-g)) goes
    subnormal (-88), and a gate whose bf16 value is 9984."""
    us = [0.5, -3.0, 100.0, 2.0 ** -10]
    ds = [1.0, -0.25, 7.0]
    rows = [(a, b, c) for a in GATES for b in us for c in ds]
    rows += [(0.0, 0.0, 0.0)] * (-len(rows) % 8)
    t = torch.tensor(rows, dtype=torch.float32).to(BF)
    _swiglu_check(t[:, 0].contiguous(), t[:, 1].contiguous(),
                  t[:, 2].contiguous())


# ------------------------------------------------------------------- xent
# fp32 chain of lse = rowmax + log(sum exp(x - rowmax)): x - rowmax is exact
# (bf16 operands), each exp is good to a few 2^-24, a thread adds at most
# 8 * ceil(V / 2048) = 16 terms, the wave and block reductions add 8 more
# levels: under 32 roundings of 2^-24 relative on the sum, 2^-19 absolute
# on its log. The log itself and the last add are each within one fp32 ulp
# of the result, 2^-18 below 32 and 2^-16 for the rows offset by 200.
# In all under 2^-15: 2^-12 leaves 8x. loss subtracts one exact bf16 logit.
def _xent_logits(gen, N, V):
    """Rows scaled so that |lse| <= 32 before the offset; odd rows carry
    +200 (the kernels must subtract the maximum first); row 2 is flat."""
    x = randn(gen, N, V) * 4.0
    if N > 2:
        x[2] = 1.5
    off = torch.zeros(N, 1)
    off[1::2] = 200.0
    base = x.to(BF)
    assert float(torch.logsumexp(base.double(), -1).abs().max()) <= 32.0
    return (x + off).to(BF)


def _xent_targets(gen, N, V):
    t = torch.randint(0, V, (N,), generator=gen)
    t[0], t[1] = 0, V - 1
    t[3::7] = -100
    return t


@pytest.mark.parametrize("N,V", [(2050, 64), (5, 8), (7, 2056)])
def test_xent_bounds(N, V):
    g = gen_of("xent", N, V)
    logits = _xent_logits(g, N, V)
    dloss = torch.rand(N, generator=g) + 0.1
    for targets in (_xent_targets(g, N, V),
                    torch.full((N,), -100, dtype=torch.long)):
        want = kc.xent_ref64(logits, targets, dloss)
        loss, lse = ops.softmax_xent_fwd(logits.to(DEV), targets.to(DEV))
        kc.assert_abs(lse, want["lse"], kc.LSE_ATOL, "xent lse")
        kc.assert_abs(loss, want["loss"], kc.LSE_ATOL, "xent loss")
        dl = ops.softmax_xent_bwd(logits.to(DEV), targets.to(DEV), lse,
                                  dloss.to(DEV))
        kc.assert_rows(dl, want["dlogits"], name="xent dlogits")
        ignored = targets == -100
        assert bool((loss.cpu()[ignored] == 0).all())
        assert bool((dl.cpu()[ignored] == 0).all())


@pytest.mark.parametrize("N,Vc", [(2050, 64), (5, 8), (7, 2056)])
def test_xent_chunk_bounds(N, Vc):
    """Three chunks whose maxima go up, then down, so the running maximum
    moves once and then holds. The target falls in chunk 0, 1, 2, in no
    chunk (a column past the three), or the row is ignored."""
    g = gen_of("xent_chunk", N, Vc)
    V = 3 * Vc
    logits = _xent_logits(g, N, V).float()
    logits[:, Vc:2 * Vc] += 6.0
    logits[:, 2 * Vc:] -= 5.0
    logits = logits.to(BF)
    r = torch.arange(N)
    cols = torch.randint(0, Vc, (N,), generator=g)
    cols[0], cols[1 % N] = 0, Vc - 1
    targets = (r % 5).clamp(max=3) * Vc + cols      # chunk 0, 1, 2, none
    targets[r % 5 == 4] = -100
    live = (targets >= 0) & (targets < V)
    want = kc.xent_ref64(logits, torch.where(live, targets, -100))

    m = torch.full((N,), -3.4e38, device=DEV)
    l = torch.zeros(N, device=DEV)
    tgt = torch.zeros(N, device=DEV)
    chunks = [logits[:, c * Vc:(c + 1) * Vc].contiguous().to(DEV)
              for c in range(3)]
    tdev = targets.to(DEV)
    for c, ch in enumerate(chunks):
        ops.xent_lse_merge(ch, tdev, m, l, tgt, c * Vc)
    lse = m.cpu().double() + l.cpu().double().log()
    kc.assert_abs(lse, want["lse"], kc.LSE_ATOL, "chunk lse")
    picked = logits.float().gather(
        1, targets.clamp(0, V - 1).unsqueeze(1)).squeeze(1)
    assert torch.equal(tgt.cpu(), torch.where(live, picked,
                                              torch.zeros(N)))
    loss = torch.where(live, lse - tgt.cpu().double(), torch.zeros(N).double())
    kc.assert_abs(loss, want["loss"], kc.LSE_ATOL, "chunk loss")

    lse_dev = m + l.log()
    for c, ch in enumerate(chunks):
        dl = ops.xent_dlogits(ch, tdev, lse_dev, c * Vc)
        ref = kc.xent_chunk_dlogits64(ch, targets, want["lse"], c * Vc)
        kc.assert_rows(dl, ref, name=f"chunk {c} dlogits")
        assert bool((dl.cpu()[targets == -100] == 0).all())


# ------------------------------------------------------------------ adamw
@pytest.mark.parametrize("n", [4, 4 * (2048 * 256 + 3)])
def test_adamw_bounds(n):
    """One kernel call per step number, each from the state the GPU holds,
    so an error cannot hide in (or be blamed on) an earlier step. The
    second size is one float4 past what 2048 blocks cover in one pass."""
    g = gen_of("adamw", n)
    hp = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)
    master = randn(g, n).to(DEV)
    m = torch.zeros(n, device=DEV)
    v = torch.zeros(n, device=DEV)
    p = torch.zeros(n, dtype=BF, device=DEV)
    for step in (1, 2, 1000):
        grad = randn(g, n)
        grad[:max(1, n // 8)] = 0.0
        if step == 1000:     # a long-run state: m and v of another scale
            m.copy_((randn(g, n) * 0.3).to(DEV))
            v.copy_((torch.rand(n, generator=g) * 2.0).to(DEV))
        before = tuple(t.cpu().clone() for t in (master, m, v))
        ops.adamw_step(p, master, grad.to(DEV), m, v, hp["lr"], hp["beta1"],
                       hp["beta2"], hp["eps"], hp["wd"], step)
        want = kc.adamw_ref64(
            before[0], grad, before[1], before[2], hp["lr"], hp["beta1"],
            hp["beta2"], hp["eps"], hp["wd"], step)
        kc.assert_elems(m, want["m"], 4 * kc.ulp32(want["mag_m"]),
                        name=f"adamw m @{step}")
        kc.assert_elems(v, want["v"], 4 * kc.ulp32(want["v"]),
                        name=f"adamw v @{step}")
        kc.assert_elems(master, want["master"],
                        2 * kc.ulp32(want["master"])
                        + 2.0 ** -20 * want["took"].abs(),
                        name=f"adamw master @{step}")
        # f2bf is round-to-nearest-even, as torch's cast is
        assert torch.equal(p, master.to(BF)), f"adamw p @{step}"


# ------------------------------------------------------ attention forward
@pytest.mark.parametrize("case", kc.ATTN_FWD_EDGE_CASES,
                         ids=lambda c: "-".join(str(int(x)) for x in c))
def test_attn_fwd_edge_shapes(case):
    B, Hq, Hkv, S, Skv, D, causal = case
    q, k, v, _ = kc.attn_inputs(B, Hq, Hkv, S, Skv, D, seed=S + Skv + D)
    want = kc.attn_ref64(q, k, v, None, causal)
    o, lse = ops.attn_fwd(q.to(DEV), k.to(DEV), v.to(DEV), causal,
                          1.0 / math.sqrt(D))
    kc.check_attn({"o": o, "lse": lse}, want, ("o",))
    assert kc.old_metric(o.cpu(), want["o"]) < 2e-2


@pytest.mark.parametrize("S", [100, 129])
def test_attn_fwd_poisoned_tail(S):
    """q/k/v are prefixes of buffers 64 rows longer whose tail is NaN: a
    read past row S that reaches the math shows up as a non-finite o."""
    B, H, D = 1, 2, 128
    q, k, v, _ = kc.attn_inputs(B, H, H, S, S, D, seed=2000 + S)
    want = kc.attn_ref64(q, k, v, None, True)

    def poisoned(t):
        buf = torch.full((B, S + 64, H, D), float("nan"), dtype=BF,
                         device=DEV)
        buf[:, :S] = t.to(DEV)
        p = buf[:, :S]
        assert p.is_contiguous()
        return p

    o, lse = ops.attn_fwd(poisoned(q), poisoned(k), poisoned(v), True,
                          1.0 / math.sqrt(D))
    assert bool(torch.isfinite(o.float()).all()), "o not finite"
    assert bool(torch.isfinite(lse).all()), "lse not finite"
    kc.check_attn({"o": o, "lse": lse}, want, ("o",))


# ------------------------------------------------- decode with len_dev
# capacity 777: two chunks of 389, so 389 / 390 straddle the chunk edge
# and length 1 leaves the second chunk empty; capacity 1100: three chunks
# of 367, lengths around 512. A length is never above the capacity.
@pytest.mark.parametrize("D,cap,lens", [
    (64, 777, [1, 389, 390]),
    (64, 777, [777, 1, 389]),
    (64, 777, [390]),
    (128, 777, [1, 389, 390]),
    (128, 777, [777, 390, 1]),
    (128, 777, [777]),
    (64, 1100, [511, 512, 513]),
    (64, 1100, [512]),
])
def test_attn_decode_len_dev(D, cap, lens):
    B, Hq, Hkv = 3, 4, 2
    assert max(lens) <= cap and min(lens) >= 1
    q, k, v, _ = kc.attn_inputs(B, Hq, Hkv, 1, cap, D, seed=cap + D)
    per_row = lens if len(lens) == B else lens * B
    for b, n in enumerate(per_row):      # the cache past each length: NaN
        k[b, n:] = float("nan")
        v[b, n:] = float("nan")
    o, lse = ops.attn_fwd(q.to(DEV), k.to(DEV), v.to(DEV), True,
                          1.0 / math.sqrt(D),
                          len_dev=torch.tensor(lens, dtype=torch.int32,
                                               device=DEV))
    assert bool(torch.isfinite(o.float()).all()), "o not finite"
    for b, n in enumerate(per_row):
        want = kc.attn_ref64(q[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n],
                             None, False)
        kc.check_attn({"o": o[b:b + 1], "lse": lse[b:b + 1]}, want, ("o",),
                      tag=f"decode row {b} len {n} ")
