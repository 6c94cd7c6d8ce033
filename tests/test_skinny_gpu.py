"""GPU tests for the bf16 weight-streaming decode GEMMs (skinny.hip):
ops.skinny_linear / skinny_linear_multi / skinny_swiglu at 1..16 rows and
the batched bf16 decode step that runs on them.

Reference: fp64 on the CPU from the same bf16 tensors. Bound, per element
(the qgemv family's, conservative here: the weights are not rounded):
    |got - want| <= 2^-7 * |want| + 2^-6 * rms(want)
SwiGLU: the swiglu `out` bound of docs/kernels.md ("Numerics bounds"),
|got - want| <= 2^-7 * |want| + 1e-30 against fp64 silu(bf16 g) * bf16 u.
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

SHAPES = [(136, 192),      # N % 16 != 0, K below one batch of 256
          (40, 264),       # K % 32 != 0: a partial k-step in batch 2
          (1032, 4096)]    # two batches per wave


def check(got, want, name):
    got, want = got.detach().double().cpu(), want.double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    tol = want.abs() * 2.0 ** -7 + want.pow(2).mean().sqrt() * 2.0 ** -6
    r = float(((got - want).abs() / tol).max())
    print(f"{name}: max err / bound = {r:.3f}")
    assert r <= 1.0, f"{name}: error is {r:.2f}x the bound"


def rand(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * 0.3).to(torch.bfloat16)


@functools.lru_cache(maxsize=8)
def case(N, K):
    """(w on the GPU, x [16,K] and residual [16,N] on the CPU, the fp64
    product [16,N]) — shared, read-only, by every M of a shape."""
    w, x, res = rand(N, K, seed=N + K), rand(16, K, seed=K), rand(16, N,
                                                                  seed=N)
    xd = x.double()
    want = torch.cat([xd @ w[i:i + 4096].double().t()
                      for i in range(0, N, 4096)], dim=1)
    return w.to(DEV), x, res, want


@pytest.mark.parametrize("M", [2, 5, 8, 16])
@pytest.mark.parametrize("N,K", SHAPES)
def test_plain_and_residual(N, K, M):
    w, x, res, want = case(N, K)
    assert ops.skinny_supported(M, N, K)
    xg = x[:M].to(DEV)
    got = ops.skinny_linear(xg, w)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (M, N)
    assert torch.equal(got, ops._EXT.skinny_gemm(xg, w))   # the kernel ran
    check(got, want[:M], f"plain M={M} N={N} K={K}")
    check(ops.skinny_linear(xg, w, res[:M].to(DEV)),
          want[:M] + res[:M].double(), f"residual M={M} N={N} K={K}")


@pytest.mark.parametrize("M", [2, 8])
def test_lm_head(M):
    """M = 2 runs the kernel (four tiles per x fragment); M = 8 at this N
    lost to the library and skinny_supported routes it back there."""
    w, x, _, want = case(32000, 4096)
    assert ops.skinny_supported(M, 32000, 4096) == (M == 2)
    check(ops.skinny_linear(x[:M].to(DEV), w), want[:M], f"lm_head M={M}")


@pytest.mark.parametrize("M", [1, 8])
def test_grouped_equals_single(M):
    x = rand(M, 192, seed=3).to(DEV)
    ws = [rand(n, 192, seed=10 + i).to(DEV)
          for i, n in enumerate((136, 40, 40))]
    outs = ops.skinny_linear_multi(x, ws)
    for w, y in zip(ws, outs):
        assert torch.equal(y, ops._EXT.skinny_gemm(x, w))
        check(y, x.double().cpu() @ w.double().cpu().t(), f"grouped M={M}")


@pytest.mark.parametrize("M", [1, 8])
def test_swiglu(M):
    wg, x, _, g64 = case(136, 192)
    wu = rand(136, 192, seed=77)
    got = ops.skinny_swiglu(x[:M].to(DEV), wg, wu.to(DEV)).double().cpu()
    g = g64[:M].to(torch.bfloat16).double()
    u = (x[:M].double() @ wu.double().t()).to(torch.bfloat16).double()
    want = g * torch.sigmoid(g) * u
    r = float(((got - want).abs() / (want.abs() * 2.0 ** -7 + 1e-30)).max())
    print(f"swiglu M={M}: max err / bound = {r:.3f}")
    assert r <= 1.0


def test_row_independence():
    """A row's bits do not depend on its batch."""
    w, x, res, _ = case(1032, 4096)
    xg, rg = x.to(DEV), res.to(DEV)
    assert torch.equal(ops.skinny_linear(xg, w)[:2],
                       ops.skinny_linear(xg[:2].contiguous(), w))
    assert torch.equal(ops.skinny_linear(xg, w, rg)[:2],
                       ops.skinny_linear(xg[:2].contiguous(), w,
                                         rg[:2].contiguous()))


def test_canary():
    """x, W and the residual are views at the front of NaN-filled buffers:
    a load past an M, N or K tail would poison the result."""
    M, N, K = 5, 136, 192
    w, x, res, want = case(N, K)

    def front(t):
        buf = torch.full((t.numel() + (1 << 15),), float("nan"), device=DEV,
                         dtype=torch.bfloat16)
        buf[:t.numel()] = t.to(DEV).reshape(-1)
        return buf[:t.numel()].view(t.shape)

    xv, wv, rv = front(x[:M]), front(w), front(res[:M])
    check(ops._EXT.skinny_gemm(xv, wv), want[:M], "canary plain")
    check(ops._EXT.skinny_gemm(xv, wv, rv), want[:M] + res[:M].double(),
          "canary residual")
    check(ops._EXT.skinny_swiglu(xv, wv, wv),
          ops.skinny_swiglu(x[:M].to(DEV), w, w), "canary swiglu")


def test_contract_and_fallback(monkeypatch):
    w, x17 = case(136, 192)[0], rand(17, 192, seed=5)
    with pytest.raises(RuntimeError):
        ops._EXT.skinny_gemm(x17.to(DEV), w)
    assert not ops.skinny_supported(17, 136, 192)
    check(ops.skinny_linear(x17.to(DEV), w),
          x17.double() @ w.double().cpu().t(), "fallback M=17")
    w68, x68 = rand(40, 68, seed=6), rand(5, 68, seed=7)
    with pytest.raises(RuntimeError):
        ops._EXT.skinny_gemm(x68.to(DEV), w68.to(DEV))
    assert not ops.skinny_supported(5, 40, 68)
    check(ops.skinny_linear(x68.to(DEV), w68.to(DEV)),
          x68.double() @ w68.double().t(), "fallback K=68")
    x = x17[:8].to(DEV)
    monkeypatch.setenv("DTX_SKINNY_GEMM", "0")
    assert torch.equal(ops.skinny_linear(x, w), F.linear(x, w))


def test_engine_batched_step_logits():
    """A bf16 tiny llama: first-step logits of the batched graphed step
    against per-request decode, within the bound. Logits, not tokens:
    the two sides sum in different orders (M = 8 MFMA vs gemv)."""
    from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
    from datatunerx_amd.serve.engine import InferenceEngine, KVCache
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
    model.eval()
    seen = {}

    def hook(_m, args, kwargs, out):
        if args[0].dim() == 2 and args[0].shape == (InferenceEngine.MAX_BATCH,
                                                    1):
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
    step_logits = seen["logits"][:, -1].float().cpu()
    for i, p in enumerate(prompts):
        caches = [KVCache(1, cfg.num_key_value_heads, 64, cfg.head_dim, DEV,
                          torch.bfloat16)
                  for _ in range(cfg.num_hidden_layers)]
        with torch.no_grad():
            model(torch.tensor([p], device=DEV), pos0=0, kv_caches=caches)
            lg = model(torch.tensor([[outs[i][0]]], device=DEV),
                       pos0=len(p), kv_caches=caches)
        check(step_logits[i], lg[0, -1].float().cpu(),
              f"batched step logits row {i}")
