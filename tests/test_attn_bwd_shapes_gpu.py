"""Backward attention at the shapes where its staging can go wrong.

The dkdv kernel loads every global row unconditionally (index clamped to
the last valid row, rows past the end zeroed by a select) and carries the
stage's lse/delta in its prefetch; dq computes delta in its prologue.
These cases sit on the edges of that scheme: less than one tile, one row
into a second 64-row stage, a second kv block, an odd stage count under
GQA, D=64 ragged, non-causal with a kv tail. Same metric and 3e-2 bound
as tests/test_ops_gpu.py::test_attn_bwd, fp32 CPU reference; beside it the
row-wise bound of tests/kernel_check.py against fp64, which also covers the
forward's o and lse at these shapes.
"""

import math

import pytest
import torch

import kernel_check as kc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from datatunerx_amd import ops
    from datatunerx_amd.ops import reference as ref
    DEV = torch.device("cuda:0")
    assert ops.have_ext(), "HIP extension must be built for GPU tests"


def mk(gen, *shape, scale=0.5):
    return (torch.randn(*shape, generator=gen, dtype=torch.float32)
            .mul(scale).to(torch.bfloat16))


def assert_close(got, want, rtol, name):
    got, want = got.float(), want.float()
    denom = want.abs().max().clamp(min=1e-3)
    err = (got - want).abs().max() / denom
    assert err < rtol, f"{name}: rel err {err:.4f} (max {denom:.3f})"


def make_case(B, Hq, Hkv, S, D, causal, seed):
    """CPU bf16 inputs, the fp32 reference gradients and the fp64
    reference with its budgets."""
    gen = torch.Generator().manual_seed(seed)
    q = mk(gen, B, S, Hq, D)
    k = mk(gen, B, S, Hkv, D)
    v = mk(gen, B, S, Hkv, D)
    do = mk(gen, B, S, Hq, D)
    o_ref, lse_ref = ref.attn_fwd(q, k, v, causal)
    grads = ref.attn_bwd(q, k, v, o_ref, do, lse_ref, causal)
    return (q, k, v, do), grads, kc.attn_ref64(q, k, v, do, causal)


def check(got, want, o, lse, want64):
    for g, w, name in zip(got, want, ("attn dq", "attn dk", "attn dv")):
        assert_close(g.cpu(), w, rtol=3e-2, name=name)
    kc.check_attn(dict(zip(("dq", "dk", "dv"), got), o=o, lse=lse), want64)


@pytest.mark.parametrize("B,Hq,Hkv,S,D,causal", [
    (1, 2, 2, 24, 128, True),        # less than one tile
    (1, 2, 2, 65, 128, True),        # one row into a second 64-row stage
    (1, 2, 2, 129, 128, True),       # second kv block of one row, qs_lo > 0
    (1, 4, 1, 192, 128, True),       # GQA rep 4, odd stage count
    (2, 2, 2, 100, 64, True),        # D=64, ragged
    (1, 2, 2, 320, 128, False),      # non-causal, 5 stages, kv tail of 64
])
def test_attn_bwd_shapes(B, Hq, Hkv, S, D, causal):
    (q, k, v, do), want, want64 = make_case(B, Hq, Hkv, S, D, causal,
                                            seed=S + D)
    q, k, v, do = (t.to(DEV) for t in (q, k, v, do))
    scale = 1.0 / math.sqrt(D)
    o, lse = ops.attn_fwd(q, k, v, causal, scale)
    got = ops.attn_bwd(q, k, v, o, do, lse, causal, scale)
    check(got, want, o, lse, want64)
    # no atomics anywhere in the backward: a second run is bit-equal
    again = ops.attn_bwd(q, k, v, o, do, lse, causal, scale)
    for a, b, name in zip(got, again, ("dq", "dk", "dv")):
        assert torch.equal(a, b), f"{name} differs between two runs"


@pytest.mark.parametrize("S", [100, 129])
def test_attn_bwd_poisoned_tail(S):
    """q/k/v/o/dO are prefixes of buffers 64 rows longer whose tail is NaN:
    a read past row S, or a clamped row that leaked into the math, shows
    up as a non-finite gradient."""
    B, H, D, causal = 1, 2, 128, True
    (q, k, v, do), want, want64 = make_case(B, H, H, S, D, causal,
                                            seed=1000 + S)
    scale = 1.0 / math.sqrt(D)
    o, lse = ops.attn_fwd(q.to(DEV), k.to(DEV), v.to(DEV), causal, scale)

    def poisoned(t):
        buf = torch.full((B, S + 64, H, D), float("nan"),
                         dtype=torch.bfloat16, device=DEV)
        buf[:, :S] = t.to(DEV)
        p = buf[:, :S]
        assert p.is_contiguous()
        return p

    qp, kp, vp, op, dop = (poisoned(t) for t in (q, k, v, o, do))
    got = ops.attn_bwd(qp, kp, vp, op, dop, lse, causal, scale)
    for g, name in zip(got, ("dq", "dk", "dv")):
        assert torch.isfinite(g.float()).all(), f"{name} not finite"
    check(got, want, o, lse, want64)
