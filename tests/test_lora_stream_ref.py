"""CPU: the reference twins of the dual LoRA ops equal the composition of
the single-adapter reference ops, so a CPU comparison of QKVProj against
unfused modules (test_fused_qkv_gateup_grads_match_unfused) still
compares like with like."""

import pytest
import torch

from datatunerx_amd import ops
from datatunerx_amd.ops import reference as ref


def _rand(g, *shape, dtype=torch.float32, scale=1.0):
    return torch.randn(*shape, generator=g).mul(scale).to(dtype)


@pytest.mark.parametrize("keep", [1.0, 0.8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_contract2_is_two_single_calls(keep, dtype):
    g = torch.Generator().manual_seed(1)
    M, K, r = 24, 32, 4
    x = _rand(g, M, K, dtype=dtype)
    w0, w1 = _rand(g, r, K, dtype=dtype), _rand(g, r, K, dtype=dtype)
    t0, t1 = ops.lora_contract2(x, w0, w1, 5, 6, keep)
    assert torch.equal(t0, ref.lora_contract(x, w0, None, 5, keep))
    assert torch.equal(t1, ref.lora_contract(x, w1, None, 6, keep))


@pytest.mark.parametrize("keep", [1.0, 0.8])
def test_expand_add2_is_two_expand_adds(keep):
    g = torch.Generator().manual_seed(2)
    M, N, r = 24, 32, 4
    t0, t1 = _rand(g, M, r), _rand(g, M, r)
    a0, a1 = _rand(g, r, N), _rand(g, r, N)
    # fp32: summing both terms before the one rounding IS the sequential
    # pair, bit for bit
    y = _rand(g, M, N)
    want = y.clone()
    ref.lora_expand_add(want, t0, a0.t(), 0.5, None, 5, keep)
    ref.lora_expand_add(want, t1, a1.t(), 0.5, None, 6, keep)
    got = ops.lora_expand_add2(y.clone(), t0, t1, a0, a1, 0.5, 5, 6, keep)
    assert torch.equal(got, want)
    # bf16: one rounding instead of two. The pair rounds the intermediate
    # y + d0 (error <= half an ulp of it, 2^-8 relative) and the final
    # sum; the dual form rounds the final sum only (2^-8 relative each).
    yb = y.to(torch.bfloat16)
    wantb = yb.clone()
    ref.lora_expand_add(wantb, t0, a0.t(), 0.5, None, 5, keep)
    inter = wantb.float().abs()
    ref.lora_expand_add(wantb, t1, a1.t(), 0.5, None, 6, keep)
    gotb = ops.lora_expand_add2(yb.clone(), t0, t1, a0, a1, 0.5, 5, 6, keep)
    # (the pair also rounds each d to bf16 before adding: 2^-8 of |d|,
    # and |d0| <= |y| + |inter|, |d1| <= |inter| + |final|)
    final = torch.maximum(wantb.float().abs(), gotb.float().abs())
    tol = 2.0 ** -8 * (yb.float().abs() + 3 * inter + 3 * final) + 1e-30
    assert ((gotb.float() - wantb.float()).abs() <= tol).all()


def test_expand_add_t_is_expand_add():
    g = torch.Generator().manual_seed(3)
    M, N, r = 16, 24, 4
    y, t, b = _rand(g, M, N), _rand(g, M, r), _rand(g, N, r)
    want = ref.lora_expand_add(y.clone(), t, b, 0.5, None, 9, 0.8)
    got = ops.lora_expand_add_t(y.clone(), t, b.t().contiguous(), 0.5,
                                None, 9, 0.8)
    assert torch.equal(got, want)
