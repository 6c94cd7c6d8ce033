"""GPU tests for the quantized decode path: the int8/int4 weight-streaming
qgemv kernels (VALU M = 1, MFMA 2 <= M <= 16), the ops.qlinear
dispatcher, the QuantFrozenLinear / QuantLoRALinear decode path and
quantized serving through the graphed decoders.

Reference: want = x.double() @ dequantize_intN(q, s, float32).double().t()
on the CPU. Acceptance bound, per element (not max-normalised):
    |got - want| <= 2^-7 * |want| + 2^-6 * rms(want)
The first term is the bf16 output rounding (2^-9) with 4x slack; the
second covers bf16-rounded weights on the MFMA int4 path (per-product
relative error 2^-9, summing randomly to ~2^-9 * rms; worst of ~5e5
outputs ~5 sigma).
"""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from datatunerx_amd import ops
    DEV = torch.device("cuda:0")
    assert ops.have_ext(), "HIP extension must be built for GPU tests"

from datatunerx_amd.models.quant import (dequantize_int4, dequantize_int8,
                                         quantize_int4, quantize_int8)

GROUP = 64


def bound_ratio(got, want):
    """max over elements of |got-want| / (2^-7 |want| + 2^-6 rms(want))."""
    got, want = got.detach().double().cpu(), want.double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.isfinite(got).all(), "non-finite output"
    rms = want.pow(2).mean().sqrt()
    tol = want.abs() * 2.0 ** -7 + rms * 2.0 ** -6
    return float(((got - want).abs() / tol).max())


def check(got, want, name):
    r = bound_ratio(got, want)
    print(f"{name}: max err / bound = {r:.3f}")
    assert r <= 1.0, f"{name}: error is {r:.2f}x the bound"


@functools.lru_cache(maxsize=8)
def weights(N, K, bits, group=GROUP):
    """(q, scale) on the GPU and the fp32 dequantized weight on the CPU
    for a seeded randn*0.3 bf16 weight; shared by the cases of a shape."""
    g = torch.Generator(device=DEV).manual_seed(1000 + N + K + bits)
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.3).to(torch.bfloat16)
    if bits == 8:
        q, s = quantize_int8(w)
        wd = dequantize_int8(q.cpu(), s.cpu(), torch.float32)
    else:
        q, s = quantize_int4(w, group)
        wd = dequantize_int4(q.cpu(), s.cpu(), torch.float32, group)
    return q, s, wd


def activations(M, K, seed=0):
    g = torch.Generator(device="cpu").manual_seed(7 + 31 * M + K + seed)
    return (torch.randn(M, K, generator=g) * 0.3).to(torch.bfloat16)


def reference(x_cpu, wd):
    """x.double() @ wd.double().t(), row-chunked to bound the fp64 copy."""
    xd = x_cpu.double()
    return torch.cat([xd @ wd[i:i + 4096].double().t()
                      for i in range(0, wd.shape[0], 4096)], dim=1)


def run_case(M, N, K, bits):
    q, s, wd = weights(N, K, bits)
    x = activations(M, K)
    assert ops.qlinear_supported(M, N, K, bits, GROUP)
    if bits == 8:
        got = ops._EXT.qgemv_int8(x.to(DEV), q, s)
    else:
        got = ops._EXT.qgemv_int4(x.to(DEV), q, s, GROUP)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (M, N)
    check(got, reference(x, wd), f"int{bits} M={M} N={N} K={K}")
    # the dispatcher takes the same kernel: bit-identical
    assert torch.equal(ops.qlinear(x.to(DEV), q, s, bits, GROUP), got)


# ------------------------------------------------------------- M = 1 (VALU)
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("N,K", [
    (121, 64),          # K below one wave step, N odd
    (264, 1088),        # one full int8 step + tail
    (264, 2112),        # one full int4 step + tail
    (1024, 11008),      # small N (1 row per wave), five full steps + tail
    (32000, 4096),      # lm_head (4 rows per wave)
])
def test_qgemv_m1(N, K, bits):
    run_case(1, N, K, bits)


# ------------------------------------------------------ 2 <= M <= 16 (MFMA)
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("M", [2, 5, 8, 16])
@pytest.mark.parametrize("N,K", [
    (136, 192),         # N % 16 != 0, K % 128 != 0
    (1032, 4096),
])
def test_qgemm_mfma(N, K, M, bits):
    run_case(M, N, K, bits)


@pytest.mark.parametrize("bits", [8, 4])
def test_qgemm_mfma_lm_head(bits):
    run_case(8, 32000, 4096, bits)


def test_qgemv_leading_dims_flatten():
    """Rows are the flattened leading dims; the output keeps them."""
    q, s, wd = weights(136, 192, 8)
    x = activations(6, 192).view(3, 2, 192)
    got = ops.qlinear(x.to(DEV), q, s, 8)
    assert tuple(got.shape) == (3, 2, 136)
    check(got.view(6, 136), reference(x.view(6, 192), wd), "leading dims")


# ------------------------------------------------------------------ canary
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("M,N,K", [(1, 121, 64), (5, 136, 192)])
def test_qgemv_canary(M, N, K, bits):
    """x, weights and scales are views at the front of larger buffers
    whose remainder is NaN (bf16/f32) or 127 (int8/uint8): a load past
    an N/K/M tail would poison the (finite, in-bound) result."""
    q, s, wd = weights(N, K, bits)
    x = activations(M, K)
    PAD = 1 << 15
    xbuf = torch.full((x.numel() + PAD,), float("nan"), device=DEV,
                      dtype=torch.bfloat16)
    xbuf[:x.numel()] = x.to(DEV).reshape(-1)
    qbuf = torch.full((q.numel() + PAD,), 127, device=DEV, dtype=q.dtype)
    qbuf[:q.numel()] = q.reshape(-1)
    sbuf = torch.full((s.numel() + PAD,), float("nan"), device=DEV,
                      dtype=torch.float32)
    sbuf[:s.numel()] = s.reshape(-1)
    xv = xbuf[:x.numel()].view(M, K)
    qv = qbuf[:q.numel()].view(q.shape)
    sv = sbuf[:s.numel()].view(s.shape)
    if bits == 8:
        got = ops._EXT.qgemv_int8(xv, qv, sv)
    else:
        got = ops._EXT.qgemv_int4(xv, qv, sv, GROUP)
    assert torch.isfinite(got.float()).all()
    check(got, reference(x, wd), f"canary int{bits} M={M}")


# ---------------------------------------------------------------- contract
@pytest.mark.parametrize("M", [1, 5])
def test_qlinear_fallback_outside_contract(M):
    """K = 72 (int8) and K = 48 (int4) are outside the kernel contract:
    ops.qlinear runs dequantize + linear and still meets the bound; the
    binding itself refuses them."""
    g = torch.Generator(device="cpu").manual_seed(5)
    w8 = (torch.randn(40, 72, generator=g) * 0.3).to(torch.bfloat16)
    q8, s8 = quantize_int8(w8)
    x8 = activations(M, 72)
    assert not ops.qlinear_supported(M, 40, 72, 8)
    got = ops.qlinear(x8.to(DEV), q8.to(DEV), s8.to(DEV), 8)
    check(got, reference(x8, dequantize_int8(q8, s8, torch.float32)),
          "fallback int8 K=72")
    with pytest.raises(RuntimeError):
        ops._EXT.qgemv_int8(x8.to(DEV), q8.to(DEV), s8.to(DEV))

    w4 = (torch.randn(40, 48, generator=g) * 0.3).to(torch.bfloat16)
    q4, s4 = quantize_int4(w4, 16)
    x4 = activations(M, 48)
    assert not ops.qlinear_supported(M, 40, 48, 4, 16)
    got = ops.qlinear(x4.to(DEV), q4.to(DEV), s4.to(DEV), 4, 16)
    check(got, reference(x4, dequantize_int4(q4, s4, torch.float32, 16)),
          "fallback int4 K=48")
    with pytest.raises(RuntimeError):
        ops._EXT.qgemv_int4(x4.to(DEV), q4.to(DEV), s4.to(DEV), 16)
    # more than 16 rows: refused by the binding, served by the fallback
    q, s, wd = weights(136, 192, 8)
    x17 = activations(17, 192)
    with pytest.raises(RuntimeError):
        ops._EXT.qgemv_int8(x17.to(DEV), q, s)
    check(ops.qlinear(x17.to(DEV), q, s, 8), reference(x17, wd),
          "fallback M=17")


# ----------------------------------------------------------------- modules
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("lora", [False, True])
def test_quant_modules_decode_path(bits, lora, monkeypatch):
    """QuantFrozenLinear / QuantLoRALinear at [1,1,K] and [8,1,K] equal
    their own F.linear(x, self.weight) (+ LoRA) evaluation, and the
    decode path never materialises the bf16 weight."""
    from datatunerx_amd.models.lora import LoRALinearModule
    from datatunerx_amd.models.quant import (QuantFrozenLinear,
                                             QuantLoRALinear)
    K, N = 256, 264
    g = torch.Generator(device="cpu").manual_seed(11 + bits)
    w = (torch.randn(N, K, generator=g) * 0.3).to(torch.bfloat16).to(DEV)
    if lora:
        with torch.device(DEV):
            src = LoRALinearModule(K, N, r=8, alpha=16.0)
        src.weight.data.copy_(w)
        src.lora_B.data.copy_(
            (torch.randn(N, 8, generator=g) * 0.3).to(torch.bfloat16))
        mod = QuantLoRALinear.from_lora(src, bits=bits)
    else:
        mod = QuantFrozenLinear.from_weight(w, bits=bits)
    prop = QuantFrozenLinear.weight
    calls = [0]

    def counted(self):
        calls[0] += 1
        return prop.fget(self)

    monkeypatch.setattr(QuantFrozenLinear, "weight", property(counted))
    for B in (1, 8):
        x = activations(B, K, seed=bits).view(B, 1, K).to(DEV)
        with torch.no_grad():
            got = mod(x)
        assert calls[0] == 0, ".weight touched on the decode path"
        assert tuple(got.shape) == (B, 1, N)
        want = F.linear(x.double(), prop.fget(mod).double())
        if lora:
            want = want + mod.lora_scale * (
                x.double() @ mod.lora_A.double().t()
            ) @ mod.lora_B.double().t()
        check(got, want, f"module int{bits} lora={lora} B={B}")
    # a call that needs a gradient keeps the dequantize + linear path
    xg = activations(2, K).to(DEV).requires_grad_(True)
    mod(xg).float().sum().backward()
    assert calls[0] >= 1 and xg.grad is not None


# ------------------------------------------------------------------ engine
def _quant_engine_model(bits):
    from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
    from datatunerx_amd.models.lora import FrozenLinear, LoRALinearModule
    from datatunerx_amd.models.quant import quantize_model_
    cfg = LlamaConfig(vocab_size=512, hidden_size=256,
                      intermediate_size=512, num_hidden_layers=2,
                      num_attention_heads=2, num_key_value_heads=2,
                      max_position_embeddings=256)
    with torch.device(DEV):
        model = LlamaForCausalLM(cfg, lora=True, dtype=torch.bfloat16)
    model.init_random(seed=3)
    g = torch.Generator(device="cpu").manual_seed(9)
    for n, p in model.named_parameters():
        if "lora_B" in n:            # a live adapter, not the zero init
            p.data.copy_((torch.randn(p.shape, generator=g) * 0.02)
                         .to(p.dtype))
    quantize_model_(model, bits, lora_base=True)
    assert not any(isinstance(m, (FrozenLinear, LoRALinearModule))
                   for m in model.modules())
    assert next(model.parameters()).dtype == torch.bfloat16
    return model.eval()


@pytest.mark.parametrize("bits", [8, 4])
def test_quant_engine_graphed_matches_eager(bits):
    from datatunerx_amd.serve.engine import InferenceEngine
    model = _quant_engine_model(bits)
    prompt = list(range(4, 24))
    eng = InferenceEngine(model, device=DEV)
    out1 = eng.generate(prompt, max_new_tokens=8)
    assert eng._graphed is not None, "graph decode did not engage"
    assert 0 < len(out1) <= 8
    eager = InferenceEngine(model, device=DEV, graph_decode=False)
    assert eager.generate(prompt, max_new_tokens=8) == out1


@pytest.mark.parametrize("bits", [8, 4])
def test_quant_engine_batched_step_logits(bits):
    """3 prompts through the batched graphed step; its first-step logits
    match the per-request decode logits (same token fed) within the
    bound. Tokens are not compared: the two sides use different kernels
    (MFMA at M = 8 vs VALU at M = 1), so near-ties may differ."""
    from datatunerx_amd.serve.engine import InferenceEngine, KVCache
    model = _quant_engine_model(bits)
    cfg = model.cfg
    seen = {}

    def hook(_m, args, kwargs, out):
        ids = args[0]
        if ids.dim() == 2 and ids.shape == (InferenceEngine.MAX_BATCH, 1):
            seen["logits"] = out     # the graph's static output buffer

    h = model.register_forward_hook(hook, with_kwargs=True)
    try:
        eng = InferenceEngine(model, device=DEV)
        prompts = [list(range(4, 24)), list(range(30, 47)),
                   list(range(60, 83))]
        outs = eng.generate_batch(prompts, max_new_tokens=2)
    finally:
        h.remove()
    assert eng._bgraphed, "batched graphed step did not engage"
    assert all(len(o) >= 1 for o in outs)
    step_logits = seen["logits"][:, -1].float().cpu()
    for i, p in enumerate(prompts):
        caches = [KVCache(1, cfg.num_key_value_heads, 64, cfg.head_dim,
                          DEV, torch.bfloat16)
                  for _ in range(cfg.num_hidden_layers)]
        with torch.no_grad():
            model(torch.tensor([p], device=DEV), pos0=0, kv_caches=caches)
            lg = model(torch.tensor([[outs[i][0]]], device=DEV),
                       pos0=len(p), kv_caches=caches)
        check(step_logits[i], lg[0, -1].float().cpu(),
              f"batched step logits int{bits} row {i}")
