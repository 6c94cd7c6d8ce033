"""The row bound of tests/kernel_check.py, checked on the CPU with no
kernel in the loop: an honest bf16 implementation (the emulation) sits
well inside it, and seeded defects that the max-norm metric lets through
land well outside it."""

import functools

import pytest
import torch

import kernel_check as kc
from datatunerx_amd.ops import reference as ref

TRAIN = kc.ATTN_BWD_CASES[-1]
assert TRAIN == (1, 2, 2, 1024, 1024, 128, True)


@functools.lru_cache(maxsize=None)
def train_case():
    """Inputs and the fp64 reference of the training shape, computed once
    and shared read-only."""
    B, Hq, Hkv, S, Skv, D, causal = TRAIN
    q, k, v, do = kc.attn_inputs(B, Hq, Hkv, S, Skv, D, seed=0)
    return (q, k, v, do), kc.attn_ref64(q, k, v, do, causal)


def emulation_ratios(case, seed):
    B, Hq, Hkv, S, Skv, D, causal = case
    if case == TRAIN and seed == 0:
        (q, k, v, do), want = train_case()
    else:
        q, k, v, do = kc.attn_inputs(B, Hq, Hkv, S, Skv, D, seed)
        want = kc.attn_ref64(q, k, v, do if S == Skv else None, causal)
    emu = kc.emulate_attn(q, k, v, do if S == Skv else None, causal)
    names = kc.ATTN_OUTPUTS if S == Skv else ("o",)
    return kc.check_attn(emu, want, names, tag=f"emulation {case} ",
                         limit=0.5)


@pytest.mark.parametrize("case", kc.ATTN_FWD_EDGE_CASES + kc.ATTN_BWD_CASES,
                         ids=lambda c: "-".join(str(int(x)) for x in c))
def test_emulation_is_inside_half_the_bound(case):
    """The condition the bound stands on: an honest bf16 implementation's
    worst row is at most 0.5 of it, for o, dq, dk and dv (and 2^-12 for
    lse). If this fails, the bound or the emulation is wrong."""
    seeds = (0,) if case == TRAIN else (0, 1, 2)
    for seed in seeds:
        emulation_ratios(case, seed)


def test_emulation_docs_case():
    """A packed batch (doc_start) through the same condition."""
    B, H, S, D = 1, 2, 200, 128
    q, k, v, do = kc.attn_inputs(B, H, H, S, S, D, seed=5)
    ds = torch.tensor([[0] * 1 + [1] * 31 + [32] * 32 + [64] * 33
                       + [97] * 64 + [161] * 39], dtype=torch.int32)
    want = kc.attn_ref64(q, k, v, do, True, doc_start=ds)
    emu = kc.emulate_attn(q, k, v, do, True, doc_start=ds)
    kc.check_attn(emu, want, tag="emulation docs ", limit=0.5)
    # the fp64 reference agrees with the fp32 twin on what is visible
    o32, lse32 = ref.attn_fwd(q, k, v, True, None, ds)
    assert kc.old_metric(o32, want["o"]) < 1e-2
    assert (lse32.double() - want["lse"]).abs().max() < 1e-4


def seeded_defect_mask(S):
    """Every q row in the bottom half loses the 8 kv columns just in front
    of its 32-column diagonal block: what a wrong interior-tile predicate
    or stage bound produces."""
    keep = torch.ones(S, S, dtype=torch.bool)
    for i in range(S // 2, S):
        b0 = (i // 32) * 32
        keep[i, max(b0 - 8, 0):b0] = False
    return keep


def test_seeded_attention_defect_passes_old_metric_fails_row_bound():
    B, Hq, Hkv, S, Skv, D, causal = TRAIN
    (q, k, v, do), want = train_case()
    bad = kc.attn_ref64(q, k, v, do, causal, extra=seeded_defect_mask(S))
    bad = {n: bad[n].to(torch.bfloat16) for n in kc.ATTN_OUTPUTS}

    # the old metric at the old limits, against the fp32 reference the
    # suite compares with: all four pass
    o32, lse32 = ref.attn_fwd(q, k, v, causal)
    g32 = ref.attn_bwd(q, k, v, o32, do, lse32, causal)
    old = {n: kc.old_metric(bad[n], w) for n, w in
           zip(kc.ATTN_OUTPUTS, (o32,) + tuple(g32))}
    print("old metric:", {n: round(x, 4) for n, x in old.items()})
    assert old["o"] < 2e-2
    for n in ("dq", "dk", "dv"):
        assert old[n] < 3e-2, (n, old[n])

    # the row bound: far outside
    new = {n: kc.row_ratio(bad[n], want[n], want["bud_" + n])
           for n in kc.ATTN_OUTPUTS}
    print("err/bound:", {n: (round(r, 2), row) for n, (r, row)
                         in new.items()})
    assert new["o"][0] > 3.0
    assert new["dq"][0] > 3.0
    assert new["dk"][0] > 10.0
    assert new["dv"][0] > 10.0
    # and the rows it names are rows the defect touched
    assert new["o"][1][1] >= S // 2 and new["dq"][1][1] >= S // 2

    # at S=128 the old metric does catch it
    q2, k2, v2, do2 = kc.attn_inputs(1, 2, 2, 128, 128, D, seed=0)
    bad2 = kc.attn_ref64(q2, k2, v2, do2, True,
                         extra=seeded_defect_mask(128))
    o2, lse2 = ref.attn_fwd(q2, k2, v2, True)
    g2 = ref.attn_bwd(q2, k2, v2, o2, do2, lse2, True)
    worst = max(kc.old_metric(bad2[n].to(torch.bfloat16), w) / lim
                for n, w, lim in zip(kc.ATTN_OUTPUTS, (o2,) + tuple(g2),
                                     (2e-2, 3e-2, 3e-2, 3e-2)))
    assert worst > 1.0


def test_truncated_xent_lse_passes_old_metric_fails_abs_bound():
    """A logsumexp that leaves the last 5 % of the vocabulary out, at the
    vocabulary of test_ops_gpu.py::test_xent. Unit-variance logits: the
    sum is then spread over the vocabulary and the loss is log(0.95) in
    every row, not the luck of where one large logit sits."""
    N, V = 32, 32000
    gen = torch.Generator().manual_seed(0)
    logits = torch.randn(N, V, generator=gen).to(torch.bfloat16)
    t = torch.randint(0, V, (N,), generator=gen)
    want = kc.xent_ref64(logits, t)
    bad = torch.logsumexp(logits[:, :V - V // 20].double(), dim=-1).float()
    _, lse32 = ref.softmax_xent_fwd(logits, t)
    assert kc.old_metric(bad, lse32) < 1e-2
    ratio, _ = kc.elem_ratio(bad, want["lse"],
                             torch.full_like(want["lse"], kc.LSE_ATOL))
    assert ratio > 10.0
    with pytest.raises(AssertionError):
        kc.assert_abs(bad, want["lse"], kc.LSE_ATOL, "truncated lse")


def test_bound_helpers_edges():
    """0/0 is inside, x/0 and NaN are outside, and the worst row is the
    one reported."""
    want = torch.zeros(3, 4, dtype=torch.float64)
    want[1] = 1.0
    got = want.clone()
    assert kc.row_ratio(got, want)[0] == 0.0
    got[0, 2] = 1e-9                       # nonzero where want is exactly 0
    assert kc.row_ratio(got, want) == (float("inf"), (0,))
    got[0, 2] = 0.0
    got[1, 0] = 1.0 + 2 * kc.C_WANT * 2.0  # row norm is 2, bound 2 * 2^-7
    r, row = kc.row_ratio(got, want)
    assert row == (1,) and abs(r - 2.0) < 1e-9
    got[2, 1] = float("nan")
    assert kc.row_ratio(got, want) == (float("inf"), (2,))
    x = torch.tensor([1.0, 1.5, 2.0, 3e-39, 0.0], dtype=torch.float64)
    assert kc.ulp32(x).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22,
                                    2.0 ** -149, 2.0 ** -149]


def test_fp64_references_agree_with_fp32_twins():
    """The new references compute the same functions as ops/reference.py
    (to fp32 accuracy), so the GPU tests did not change what they ask for,
    only how precisely."""
    gen = torch.Generator().manual_seed(3)
    rn = lambda *s: torch.randn(*s, generator=gen)
    x, w, dy, dres = (rn(5, 64).bfloat16(), rn(64).bfloat16(),
                      rn(5, 64).bfloat16(), rn(5, 64).bfloat16())
    r = kc.rmsnorm_ref64(x, w, 1e-5, dy, dres)
    y32, inv32 = ref.rmsnorm_fwd(x.float(), w.float(), 1e-5)
    dx32, dw32 = ref.rmsnorm_bwd(dy.float(), x.float(), w.float(), inv32)
    for a, b in ((r["y"], y32), (r["inv"], inv32),
                 (r["dx"], dx32 + dres.float()), (r["dw"], dw32)):
        assert torch.allclose(a.float(), b, rtol=1e-5, atol=1e-5)

    cos, sin = ref.rope_tables(32, 64)
    xr = rn(2, 5, 2, 64).bfloat16()
    pos = torch.tensor([[3 + s for s in range(5)]] * 2)
    for bwd, f in ((False, ref.rope_fwd), (True, ref.rope_bwd)):
        y, _ = kc.rope_ref64(xr, cos, sin, pos, backward=bwd)
        assert torch.allclose(y.float(), f(xr.float(), cos, sin, 3),
                              rtol=1e-5, atol=1e-6)

    g, u, d = rn(4, 16).bfloat16(), rn(4, 16).bfloat16(), rn(4, 16).bfloat16()
    s = kc.swiglu_ref64(g, u, d)
    dg32, du32 = ref.swiglu_bwd(d.float(), g.float(), u.float())
    assert torch.allclose(s["out"].float(),
                          ref.swiglu_fwd(g.float(), u.float()), atol=1e-6)
    assert torch.allclose(s["dg"].float(), dg32, atol=1e-6)
    assert torch.allclose(s["du"].float(), du32, atol=1e-6)
    assert bool((s["bud_dg"] >= s["dg"].abs() - 1e-15).all())

    logits = rn(6, 24).bfloat16()
    t = torch.tensor([0, 23, -100, 5, 7, 8])
    dloss = torch.rand(6, generator=gen)
    xr64 = kc.xent_ref64(logits, t, dloss)
    loss32, lse32 = ref.softmax_xent_fwd(logits, t)
    dl32 = ref.softmax_xent_bwd(logits.float(), t, lse32, dloss)
    assert torch.allclose(xr64["loss"].float(), loss32, atol=1e-5)
    assert torch.allclose(xr64["dlogits"].float(), dl32, atol=1e-6)
    ch = kc.xent_chunk_dlogits64(logits[:, 8:16], t, xr64["lse"], 8)
    ch32 = ref.xent_dlogits(logits[:, 8:16].float(), t, lse32, 8)
    assert torch.allclose(ch.float(), ch32, atol=1e-6)

    n = 16
    p0, g0, m0 = rn(n), rn(n), rn(n) * 0.1
    v0 = torch.rand(n, generator=gen) * 0.01
    args = (1e-3, 0.9, 0.999, 1e-8, 0.01, 2)
    a64 = kc.adamw_ref64(p0, g0, m0, v0, *args)
    p64, m64, v64, took = (a64[n] for n in ("master", "m", "v", "took"))
    assert bool((a64["mag_m"] >= m64.abs()).all())
    pb, pm, mm, vv = p0.bfloat16(), p0.clone(), m0.clone(), v0.clone()
    ref.adamw_step(pb, pm, g0, mm, vv, *args)
    assert torch.allclose(p64.float(), pm, rtol=1e-5, atol=1e-7)
    # 1 - fp32(0.999) is 1.00005e-3: the fp32 twin takes 1e-3 from the
    # Python float, the kernel and the fp64 reference the fp32 difference
    assert torch.allclose(m64.float(), mm, rtol=1e-6)
    assert torch.allclose(v64.float(), vv, rtol=1e-4)
    assert torch.allclose((p0.double() * (1 - 1e-5) - took).float(), pm,
                          rtol=1e-5, atol=1e-7)
