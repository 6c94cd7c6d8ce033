"""GPU tests for NF4 base weights: the bulk dequant kernel (bit-identical
to the CPU reference), the weight-streaming decode kernels (VALU M = 1,
MFMA 2 <= M <= 16), the ops.qlinear route, the module decode path and
NF4 serving through the graphed decoder.

Reference: want = x.double() @ dequantize_nf4(q, a, float32).double().t()
on the CPU, and A = |x|.double() @ |wd|.double().t(). Acceptance bound,
per element, derived:
    |got - want| <= (2^-8 + 2^-11) * A + 2^-8 * |want|
2^-8 * A: the kernels feed bf16-rounded levels (unit roundoff 2^-8);
2^-11 * A: fp32 accumulation up to K = 4096; 2^-8 * |want|: the bf16
output rounding. A wrong nibble order, group or tail is an error of about
rms(want), 6-50x this bound at K = 4096-64.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from datatunerx_amd import ops
    DEV = torch.device("cuda:0")
    assert ops.have_ext(), "HIP extension must be built for GPU tests"

from datatunerx_amd.models.quant import dequantize_nf4, quantize_nf4


def check(got, x_cpu, wd, name, extra=None):
    """extra: (value, sum of absolute products) of a further fp64 term of
    the reference (a LoRA branch), added to want and to A."""
    xd, wdd = x_cpu.double(), wd.double()
    want, A = xd @ wdd.t(), xd.abs() @ wdd.abs().t()
    if extra is not None:
        want, A = want + extra[0], A + extra[1]
    got = got.detach().double().cpu().view(want.shape)
    assert torch.isfinite(got).all(), "non-finite output"
    tol = (2.0 ** -8 + 2.0 ** -11) * A + 2.0 ** -8 * want.abs()
    r = float(((got - want).abs() / tol).max())
    print(f"{name}: max err / bound = {r:.3f}")
    assert r <= 1.0, f"{name}: error is {r:.2f}x the bound"


@functools.lru_cache(maxsize=None)
def weights(N, K, group=64):
    """(packed, absmax) on the GPU and the fp32 dequantized weight on the
    CPU for a seeded randn*0.3 bf16 weight; shared by a shape's cases."""
    g = torch.Generator(device=DEV).manual_seed(1000 + N + K + group)
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.3).to(torch.bfloat16)
    q, a = quantize_nf4(w, group)
    return q, a, dequantize_nf4(q.cpu(), a.cpu(), torch.float32, group)


def activations(M, K, seed=0):
    g = torch.Generator(device="cpu").manual_seed(7 + 31 * M + K + seed)
    return (torch.randn(M, K, generator=g) * 0.3).to(torch.bfloat16)


@pytest.mark.parametrize("N,K,group", [(8, 64, 64), (121, 192, 64),
                                       (8, 64, 32), (40, 48, 16)])
def test_dequant_nf4_bit_identical(N, K, group):
    q, a, _ = weights(N, K, group)
    got = ops.dequant_nf4(q, a, group)
    want = dequantize_nf4(q.cpu(), a.cpu(), torch.bfloat16, group)
    assert got.dtype == torch.bfloat16
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("M", [1, 2, 5, 16])
@pytest.mark.parametrize("N,K,group", [
    (121, 64, 64),          # K below one wave step, N odd
    (264, 2112, 64),        # one full M = 1 step + tail
    (136, 192, 64),         # N % 16 != 0, K % 128 != 0
    (1032, 4096, 64),
    (136, 384, 32),         # one scale group per piece (GPS 4)
    (136, 384, 128),        # one scale group per wave step (GPS 1)
])
def test_qgemv_nf4(N, K, group, M):
    q, a, wd = weights(N, K, group)
    x = activations(M, K)
    got = ops._EXT.qgemv_nf4(x.to(DEV), q, a, group)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (M, N)
    check(got, x, wd, f"nf4 M={M} N={N} K={K} g={group}")
    # the dispatcher takes the same kernel: bit-identical
    assert torch.equal(ops.qlinear(x.to(DEV), q, a, 4, group, "nf4"), got)


@pytest.mark.parametrize("M,N,K", [(1, 121, 64), (5, 136, 192)])
def test_qgemv_nf4_canary(M, N, K):
    """x, weights and absmax are views at the front of larger buffers
    whose remainder is NaN (bf16/f32) or 127 (uint8): a load past an
    N/K/M tail would poison the (finite, in-bound) result."""
    q, a, wd = weights(N, K)
    x = activations(M, K)
    PAD = 1 << 15
    xbuf = torch.full((x.numel() + PAD,), float("nan"), device=DEV,
                      dtype=torch.bfloat16)
    xbuf[:x.numel()] = x.to(DEV).reshape(-1)
    qbuf = torch.full((q.numel() + PAD,), 127, device=DEV, dtype=q.dtype)
    qbuf[:q.numel()] = q.reshape(-1)
    abuf = torch.full((a.numel() + PAD,), float("nan"), device=DEV,
                      dtype=torch.float32)
    abuf[:a.numel()] = a.reshape(-1)
    got = ops._EXT.qgemv_nf4(xbuf[:x.numel()].view(M, K),
                             qbuf[:q.numel()].view(q.shape),
                             abuf[:a.numel()].view(a.shape), 64)
    check(got, x, wd, f"canary nf4 M={M}")


@pytest.mark.parametrize("M", [1, 5])
def test_qlinear_nf4_fallback_outside_contract(M):
    """K = 48 with group 16 is outside the kernel contract: ops.qlinear
    runs dequant_nf4 + linear; the binding itself refuses it."""
    q, a, wd = weights(40, 48, 16)
    x = activations(M, 48)
    assert not ops.qlinear_supported(M, 40, 48, 4, 16)
    check(ops.qlinear(x.to(DEV), q, a, 4, 16, "nf4"), x, wd,
          "fallback nf4 K=48")
    with pytest.raises(RuntimeError):
        ops._EXT.qgemv_nf4(x.to(DEV), q, a, 16)


@pytest.mark.parametrize("B", [1, 5])
def test_quant_lora_nf4_decode_vs_prefill(B):
    """QuantLoRALinear(codebook="nf4") at B rows (the decode kernels)
    against its own dequantized weight plus the LoRA branch in fp64."""
    from datatunerx_amd.models.lora import LoRALinearModule
    from datatunerx_amd.models.quant import QuantLoRALinear
    K, N = 256, 264
    g = torch.Generator(device="cpu").manual_seed(15)
    with torch.device(DEV):
        src = LoRALinearModule(K, N, r=8, alpha=16.0)
    src.weight.data.copy_((torch.randn(N, K, generator=g) * 0.3)
                          .to(torch.bfloat16))
    src.lora_B.data.copy_((torch.randn(N, 8, generator=g) * 0.3)
                          .to(torch.bfloat16))
    mod = QuantLoRALinear.from_lora(src, bits=4, codebook="nf4")
    assert mod.codebook == "nf4"
    x = activations(B, K, seed=4)
    xg = x.view(B, 1, K).to(DEV)
    assert mod._decode_path(xg)
    with torch.no_grad():
        got = mod(xg)
    assert tuple(got.shape) == (B, 1, N)
    wd = dequantize_nf4(mod.qweight.cpu(), mod.scale.cpu(), torch.float32)
    assert torch.equal(mod.weight.cpu(), wd.to(torch.bfloat16))
    la, lb = mod.lora_A.double().cpu().t(), mod.lora_B.double().cpu().t()
    lora = (mod.lora_scale * (x.double() @ la) @ lb,
            mod.lora_scale * (x.double().abs() @ la.abs()) @ lb.abs())
    check(got, x, wd, f"module nf4 B={B}", extra=lora)


def test_nf4_engine_graphed_decode():
    """llama-tiny's head size is outside the GPU attention kernels, so
    the model is the two-layer one of tests/test_qgemv_gpu.py (D = 128)."""
    from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
    from datatunerx_amd.models.quant import (QuantFrozenLinear,
                                             quantize_model_)
    from datatunerx_amd.serve.engine import InferenceEngine
    cfg = LlamaConfig(vocab_size=512, hidden_size=256,
                      intermediate_size=512, num_hidden_layers=2,
                      num_attention_heads=2, num_key_value_heads=2,
                      max_position_embeddings=256)
    with torch.device(DEV):
        model = LlamaForCausalLM(cfg, lora=True, dtype=torch.bfloat16)
    model.init_random(seed=3)
    quantize_model_(model, 4, lora_base=True, codebook="nf4")
    model.eval()
    quant = [m for m in model.modules() if isinstance(m, QuantFrozenLinear)]
    assert quant and all(m.codebook == "nf4" for m in quant)
    prompt = list(range(4, 24))
    eng = InferenceEngine(model, device=DEV)
    out = eng.generate(prompt, max_new_tokens=8)
    assert eng._graphed is not None, "graph decode did not engage"
    assert 0 < len(out) <= 8
    assert eng.generate(prompt, max_new_tokens=8) == out
