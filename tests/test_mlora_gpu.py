"""GPU tests for multi-adapter decode: the gathered LoRA kernels
(mlora.hip) behind ops.mlora_add, MultiLoRALinear over bf16 / int8 / int4
bases, and per-request adapters through the graphed decoders.

Reference, on the CPU in float64 from the bf16 inputs:
    want[m] = y[m] + scale[g] * (x[m] @ A[g]^T) @ Bt[g],   g = idx[m]
Acceptance bound, per element (the project's bound, test_qgemv_gpu.py):
    |got - want| <= 2^-7 * |want| + 2^-6 * rms(want)
The first term is the bf16 output rounding (2^-9) with 4x slack; the
second is generous here because every accumulation is fp32.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from datatunerx_amd import ops
    DEV = torch.device("cuda:0")
    assert ops.have_ext(), "HIP extension must be built for GPU tests"

G = 5
SCALES = (4.0, 2.0, 0.5, 4.0, 2.0)


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


@functools.lru_cache(maxsize=4)
def stack(K, N, R):
    """Seeded adapter stack (A [G,R,K], Bt [G,R,N] randn*0.05 bf16,
    scale [G]) on the CPU and on the GPU; shared by a shape's cases."""
    g = torch.Generator().manual_seed(100 + K + N + R)
    A = (torch.randn(G, R, K, generator=g) * 0.05).to(torch.bfloat16)
    Bt = (torch.randn(G, R, N, generator=g) * 0.05).to(torch.bfloat16)
    s = torch.tensor(SCALES, dtype=torch.float32)
    return (A, Bt, s), (A.to(DEV), Bt.to(DEV), s.to(DEV))


def rows(M, K, N, seed=0):
    g = torch.Generator().manual_seed(7 + 31 * M + K + N + seed)
    x = (torch.randn(M, K, generator=g) * 0.3).to(torch.bfloat16)
    y = (torch.randn(M, N, generator=g) * 0.3).to(torch.bfloat16)
    return x, y


def pattern(kind, M):
    if kind == "equal":
        return [2] * M
    if kind == "cycle":
        return [m % G for m in range(M)]
    # mixed: some rows on the base model
    return [-1 if m % 3 == 1 else (2 * m + 1) % G for m in range(M)]


def reference(y, x, A, Bt, s, idx):
    want = y.double().clone()
    for m, g in enumerate(idx):
        if 0 <= g < A.shape[0]:
            want[m] += s[g].double() * (
                x[m].double() @ A[g].double().t()) @ Bt[g].double()
    return want


def run(y, x, dev_stack, idx):
    out = y.to(DEV)
    ret = ops.mlora_add(out, x.to(DEV), *dev_stack,
                        torch.tensor(idx, dtype=torch.int32, device=DEV))
    assert ret is out
    return out


# --------------------------------------------------------------- numerics
@pytest.mark.parametrize("kind", ["equal", "cycle", "mixed"])
@pytest.mark.parametrize("M", [1, 3, 8, 16])
@pytest.mark.parametrize("K,N,R", [
    (64, 72, 8),            # K below one wave step, N tail
    (1088, 264, 16),
    (4096, 1024, 16),       # GQA v_proj
    (11008, 4096, 64),      # longest K, widest R
])
def test_mlora_kernel(K, N, R, M, kind):
    cpu, dev = stack(K, N, R)
    x, y = rows(M, K, N)
    idx = pattern(kind, M)
    assert ops.mlora_supported(M, N, K, R)
    got = run(y, x, dev, idx)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (M, N)
    check(got, reference(y, x, *cpu, idx),
          f"mlora K={K} N={N} R={R} M={M} {kind}")
    for m, g in enumerate(idx):
        if g < 0:
            assert torch.equal(got[m].cpu(), y[m]), f"row {m} was touched"


# --------------------------------------------------------- untouched rows
@pytest.mark.parametrize("K,N,R", [(64, 72, 8), (4096, 1024, 16)])
def test_mlora_rows_without_adapter_are_untouched(K, N, R):
    _cpu, dev = stack(K, N, R)
    x, y = rows(8, K, N, seed=1)
    assert torch.equal(run(y, x, dev, [-1] * 8).cpu(), y)
    # an index past the stack is a memory-safety guard: skipped as well
    assert torch.equal(run(y, x, dev, [G, -7, 1 << 30, G + 1] * 2).cpu(), y)


# ------------------------------------------------------- row independence
@pytest.mark.parametrize("K,N,R", [(1088, 264, 16), (11008, 4096, 64)])
def test_mlora_row_depends_on_that_row_only(K, N, R):
    """Row m of a mixed batch is bitwise the same row run alone."""
    _cpu, dev = stack(K, N, R)
    x, y = rows(8, K, N, seed=2)
    idx = pattern("mixed", 8)
    got = run(y, x, dev, idx)
    for m in range(8):
        alone = run(y[m:m + 1], x[m:m + 1], dev, idx[m:m + 1])
        assert torch.equal(alone[0], got[m]), f"row {m} differs"
    # and of the other rows' adapters
    other = run(y, x, dev, [idx[0]] + [4] * 7)
    assert torch.equal(other[0], got[0])


# ------------------------------------------------------------ rank padding
@pytest.mark.parametrize("R", [16, 64])
def test_mlora_rank_padding_is_bitwise(R):
    """An r = 8 adapter zero-padded into an R = 16 / 64 stack gives the
    same bits as in an R = 8 stack: the shrink sums each rank the same
    way whatever R is, and the expand adds ranks in one chain, so the
    padding only adds exact zeros."""
    K, N = 1088, 264
    (A8, Bt8, s), dev8 = stack(K, N, 8)
    A = torch.zeros(G, R, K, dtype=torch.bfloat16)
    Bt = torch.zeros(G, R, N, dtype=torch.bfloat16)
    A[:, :8], Bt[:, :8] = A8, Bt8
    x, y = rows(8, K, N, seed=3)
    idx = pattern("cycle", 8)
    got8 = run(y, x, dev8, idx)
    gotR = run(y, x, (A.to(DEV), Bt.to(DEV), s.to(DEV)), idx)
    assert torch.equal(got8, gotR)
    check(gotR, reference(y, x, A8, Bt8, s, idx), f"padded to R={R}")


def test_mlora_add_refuses_outside_contract():
    _cpu, (A, Bt, s) = stack(64, 72, 8)
    x, y = rows(17, 64, 72)
    idx = torch.zeros(17, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="contract"):
        ops.mlora_add(y.to(DEV), x.to(DEV), A, Bt, s, idx)
    with pytest.raises(ValueError):          # idx on the host
        ops.mlora_add(y[:2].to(DEV), x[:2].to(DEV), A, Bt, s,
                      torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError):        # the binding checks too
        ops._EXT.mlora_add(y.to(DEV), x.to(DEV), A, Bt, s, idx)


# ------------------------------------------------------------------ module
@pytest.mark.parametrize("base_kind", ["bf16", "int8", "int4"])
def test_multilora_module(base_kind):
    from datatunerx_amd.models.lora import FrozenLinear
    from datatunerx_amd.models.multilora import (AdapterSelection,
                                                 MultiLoRALinear)
    from datatunerx_amd.models.quant import QuantFrozenLinear
    K, N = 256, 264
    g = torch.Generator().manual_seed(21)
    with torch.device(DEV):
        base = FrozenLinear(K, N)
    base.weight.data.copy_(
        (torch.randn(N, K, generator=g) * 0.3).to(torch.bfloat16))
    if base_kind != "bf16":
        base = QuantFrozenLinear.from_weight(
            base.weight.detach(), bits=8 if base_kind == "int8" else 4)
    mod = MultiLoRALinear(base, 3, 16)
    specs = [(8, 4.0), (16, 2.0), (8, 0.5)]
    for i, (r, sc) in enumerate(specs):
        mod.set_adapter(
            i, (torch.randn(r, K, generator=g) * 0.05).to(torch.bfloat16),
            (torch.randn(N, r, generator=g) * 0.05).to(torch.bfloat16), sc)
    A, Bt = mod.A.double().cpu(), mod.Bt.double().cpu()

    def want_for(x, idx):
        with torch.no_grad():
            w = mod.base(x).double().cpu()
        for b, gi in enumerate(idx):
            if gi >= 0:
                w[b] += specs[gi][1] * (x[b].double().cpu() @ A[gi].t()) \
                    @ Bt[gi]
        return w

    for B, S, idx in ((1, 1, [1]), (8, 1, [0, -1, 2, 1, 1, -1, 0, 2]),
                      (2, 5, [2, 1]), (2, 5, [-1, 0])):
        x = (torch.randn(B, S, K, generator=g) * 0.3).to(torch.bfloat16) \
            .to(DEV)
        sel = AdapterSelection(
            torch.tensor(idx, dtype=torch.int32, device=DEV), idx)
        with torch.no_grad():
            got = mod(x, adapters=sel)
            assert torch.equal(mod(x), mod.base(x))
        assert tuple(got.shape) == (B, S, N)
        check(got, want_for(x, idx), f"module {base_kind} [{B},{S},K]")
        if S == 1:
            # decode reads the device indices only
            with torch.no_grad():
                dev_only = mod(x, adapters=AdapterSelection(sel.dev, None))
            assert torch.equal(dev_only, got)
            res = (torch.randn(B, S, N, generator=g) * 0.3) \
                .to(torch.bfloat16).to(DEV)
            with torch.no_grad():
                with_res = mod(x, adapters=sel, residual=res)
            check(with_res, want_for(x, idx) + res.double().cpu(),
                  f"module {base_kind} [{B},{S},K] + residual")


# ------------------------------------------------------------------ engine
ADAPTERS = {
    "a": (8, 32.0, ("q_proj", "v_proj")),
    "b": (16, 32.0, ("q_proj", "v_proj")),
    "c": (8, 16.0, ("q_proj", "k_proj", "v_proj", "o_proj", "down_proj")),
}


def _cfg(**kw):
    from datatunerx_amd.models import LlamaConfig
    return LlamaConfig(vocab_size=512, hidden_size=256,
                       intermediate_size=512, num_hidden_layers=2,
                       num_attention_heads=2, num_key_value_heads=2,
                       max_position_embeddings=256, **kw)


def _base_state():
    from datatunerx_amd.models import LlamaForCausalLM
    with torch.device(DEV):
        m = LlamaForCausalLM(_cfg(), lora=False, dtype=torch.bfloat16)
    m.init_random(seed=3)
    return {k: v.clone() for k, v in m.state_dict().items()}


def _write_adapters(root):
    from datatunerx_amd.models import LlamaForCausalLM, save_adapter
    dirs = {}
    for i, (name, (r, alpha, targets)) in enumerate(ADAPTERS.items()):
        m = LlamaForCausalLM(_cfg(lora_r=r, lora_alpha=alpha,
                                  lora_targets=targets),
                             lora=True, dtype=torch.bfloat16)
        g = torch.Generator().manual_seed(40 + i)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if "lora_A" in n or "lora_B" in n:
                    p.copy_((torch.randn(p.shape, generator=g) * 0.02)
                            .to(p.dtype))
        dirs[name] = str(root / name)
        save_adapter(m, dirs[name], r=r, alpha=alpha, dropout=0.0,
                     target_modules=list(targets))
    return dirs


def _model(base_sd, bits, name=None, dirs=None, multi=False):
    """multi: all adapters attached as stacks; name: that one adapter the
    existing single-adapter way (LoRALinearModule); neither: no adapter.
    Every variant carries the same base weights."""
    from datatunerx_amd.models import LlamaForCausalLM, load_adapter
    from datatunerx_amd.models.multilora import attach_adapters_
    from datatunerx_amd.models.quant import quantize_model_
    kw = {}
    if name is not None:
        r, alpha, targets = ADAPTERS[name]
        kw = dict(lora_r=r, lora_alpha=alpha, lora_targets=targets)
    with torch.device(DEV):
        m = LlamaForCausalLM(_cfg(**kw), lora=name is not None,
                             dtype=torch.bfloat16)
    missing, unexpected = m.load_state_dict(base_sd, strict=False)
    assert not unexpected and all("lora_" in k for k in missing)
    if name is not None:
        assert load_adapter(m, dirs[name]) > 0
    if multi:
        attach_adapters_(m, dirs)
    if bits:
        quantize_model_(m, bits, lora_base=True)
    return m.eval()


def _decode_logits(model, prompt, tok):
    """Eager single-request logits after `prompt` + `tok`."""
    from datatunerx_amd.serve.engine import KVCache
    cfg = model.cfg
    caches = [KVCache(1, cfg.num_key_value_heads, 64, cfg.head_dim, DEV,
                      torch.bfloat16)
              for _ in range(cfg.num_hidden_layers)]
    with torch.no_grad():
        model(torch.tensor([prompt], device=DEV), pos0=0, kv_caches=caches)
        lg = model(torch.tensor([[tok]], device=DEV), pos0=len(prompt),
                   kv_caches=caches)
    return lg[0, -1].float().cpu()


@pytest.mark.parametrize("bits", [0, 8])
def test_engine_graphed_adapter_per_row(bits, tmp_path):
    """One captured batched step serves every assignment of adapters:
    its logits match, row by row, the eager decode logits of a model
    carrying only that row's adapter the single-adapter way — and still
    do after the assignment changes on the SAME graph (the index is read
    at replay). Tokens are not compared across models (near-ties)."""
    from datatunerx_amd.serve.engine import InferenceEngine
    base_sd = _base_state()
    dirs = _write_adapters(tmp_path)
    multi = _model(base_sd, bits, dirs=dirs, multi=True)
    refs = {n: _model(base_sd, bits, name=n, dirs=dirs)
            for n in ("a", "c")}
    refs[None] = _model(base_sd, bits)
    seen = {}

    def hook(_m, args, kwargs, out):
        ids = args[0]
        if ids.dim() == 2 and ids.shape == (InferenceEngine.MAX_BATCH, 1):
            seen["logits"] = out     # the graph's static output buffer

    prompts = [list(range(4, 24)), list(range(30, 47)),
               list(range(60, 83))]
    h = multi.register_forward_hook(hook, with_kwargs=True)
    try:
        eng = InferenceEngine(multi, device=DEV)
        graph = None
        for names in (["a", None, "c"], ["c", "a", None]):
            outs = eng.generate_batch(prompts, max_new_tokens=2,
                                      adapters=names)
            assert eng._bgraphed, "batched graphed step did not engage"
            if graph is None:
                graph = eng._bgraphed
            assert eng._bgraphed is graph, "the graph was rebuilt"
            assert all(len(o) >= 1 for o in outs)
            step_logits = seen["logits"][:, -1].float().cpu()
            for i, (p, n) in enumerate(zip(prompts, names)):
                tok = outs[i][0]
                check(step_logits[i], _decode_logits(refs[n], p, tok),
                      f"bits={bits} {names} row {i} ({n})")
                if n is not None:
                    # ... and NOT the base model's: the adapter counts
                    assert bound_ratio(
                        step_logits[i],
                        _decode_logits(refs[None], p, tok)) > 1.0
    finally:
        h.remove()
    # single stream: graphed == eager on the same model (same kernels)
    prompt = prompts[0]
    for n in ("a", None, "c"):
        out = eng.generate(prompt, max_new_tokens=8, adapter=n)
        assert eng._graphed is not None, "graph decode did not engage"
        assert 0 < len(out) <= 8
        eager = InferenceEngine(multi, device=DEV, graph_decode=False)
        assert eager.generate(prompt, max_new_tokens=8, adapter=n) == out
