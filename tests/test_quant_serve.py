"""CPU tests for quantized serving: the ops.qlinear dispatcher, the
QuantFrozenLinear / QuantLoRALinear modules, quantize_model_(lora_base),
build_model(quantization=...), the server flag and the
serveConfig.quantization CR field down to the spawned serve command."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from datatunerx_amd import ops
from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
from datatunerx_amd.models.lora import FrozenLinear, LoRALinearModule
from datatunerx_amd.models.quant import (QuantFrozenLinear, QuantLoRALinear,
                                         dequantize_int4, dequantize_int8,
                                         quantize_int4, quantize_int8,
                                         quantize_model_)


def _quant(w, bits, group):
    if bits == 8:
        q, s = quantize_int8(w)
        return q, s, dequantize_int8(q, s, torch.float32)
    q, s = quantize_int4(w, group)
    return q, s, dequantize_int4(q, s, torch.float32, group)


# --------------------------------------------------------------- dispatcher
@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("bits,K,group", [
    (8, 128, 64), (4, 128, 64),
    (8, 72, 64),        # K % 16 != 0: outside the GPU kernel contract
    (4, 48, 16),        # K % 32 != 0, group % 32 != 0
])
def test_qlinear_cpu_is_fp32_reference(M, bits, K, group):
    torch.manual_seed(0)
    w = torch.randn(24, K) * 0.3
    q, s, wd = _quant(w, bits, group)
    x = torch.randn(M, K)
    got = ops.qlinear(x, q, s, bits, group)
    assert got.dtype == x.dtype and tuple(got.shape) == (M, 24)
    assert torch.equal(got, (x.float() @ wd.t()).to(x.dtype))
    # leading dims are kept; bf16 activations come back as bf16
    xb = x.to(torch.bfloat16).view(M, 1, K)
    gb = ops.qlinear(xb, q, s, bits, group)
    assert gb.dtype == torch.bfloat16 and tuple(gb.shape) == (M, 1, 24)
    assert torch.equal(gb, (xb.float() @ wd.t()).to(torch.bfloat16))


def test_qlinear_supported_contract():
    sup = ops.qlinear_supported
    assert sup(1, 4096, 4096, 8) and sup(16, 121, 64, 4, 64)
    assert not sup(17, 4096, 4096, 8)        # more than 16 rows
    assert not sup(0, 4096, 4096, 8)
    assert not sup(1, 40, 72, 8)             # K % 16
    assert not sup(1, 40, 48, 4, 16)         # K % 32, group % 32
    assert not sup(1, 40, 64, 4, 16)         # group % 32
    assert sup(1, 40, 96, 4, 32)
    assert not sup(1, 40, 64, 3)
    with pytest.raises(ValueError):
        ops.qlinear(torch.zeros(1, 64), torch.zeros(4, 64, dtype=torch.int8),
                    torch.ones(4), 3)


# ------------------------------------------------------------------ modules
@pytest.mark.parametrize("bits", [8, 4])
def test_quant_frozen_linear_cpu_paths_unchanged(bits):
    """Decode-shaped forward under no_grad gives F.linear(x, weight) as
    before; an input that needs a gradient still back-propagates."""
    torch.manual_seed(1)
    m = QuantFrozenLinear.from_weight(torch.randn(48, 128) * 0.3, bits=bits)
    x = torch.randn(1, 1, 128)
    with torch.no_grad():
        y = m(x)
    assert torch.equal(y, F.linear(x, m.weight))
    xg = torch.randn(3, 128, requires_grad=True)
    m(xg).sum().backward()
    assert torch.allclose(xg.grad, m.weight.sum(0).expand(3, -1), atol=1e-5)


def _tiny_lora_model(seed=0):
    cfg = LlamaConfig.tiny()
    model = LlamaForCausalLM(cfg, lora=True, dtype=torch.float32)
    model.init_random(seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    for n, p in model.named_parameters():
        if "lora_B" in n:            # a live adapter, not the zero init
            p.data.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return model.eval()


def _proj_bytes(model):
    kinds = (FrozenLinear, LoRALinearModule, QuantFrozenLinear)
    total = 0
    for m in model.modules():
        if isinstance(m, kinds):
            for name, t in list(m.named_parameters(recurse=False)) + \
                    list(m.named_buffers(recurse=False)):
                if not name.startswith("lora_"):
                    total += t.numel() * t.element_size()
    return total


@pytest.mark.parametrize("bits", [8, 4])
def test_quantize_model_lora_base(bits):
    model = _tiny_lora_model()
    ref = _tiny_lora_model()
    assert any(isinstance(m, LoRALinearModule) for m in model.modules())
    base_elems = _proj_bytes(model) // 4         # fp32 base weights
    n = quantize_model_(model, bits, lora_base=True)
    n_proj = sum(isinstance(m, (FrozenLinear, LoRALinearModule))
                 for m in ref.modules())
    assert n == n_proj
    assert not any(isinstance(m, (FrozenLinear, LoRALinearModule))
                   for m in model.modules())
    assert any(isinstance(m, QuantLoRALinear) for m in model.modules())
    # bytes at rest: bits/16 of bf16 plus the f32 scales (one per 64
    # weights for int4 = 1/32 of bf16 bytes; one per row for int8)
    bf16_bytes = 2 * base_elems
    overhead = 1.0 / 32 if bits == 4 else 4.0 / (2 * 128)
    assert _proj_bytes(model) <= (bits / 16 + overhead) * bf16_bytes
    # adapter survives: logits equal those of the unquantized model whose
    # base weights were replaced by their dequantized values
    qmods = dict(model.named_modules())
    with torch.no_grad():
        for name, m in ref.named_modules():
            if isinstance(m, (FrozenLinear, LoRALinearModule)):
                m.weight.copy_(qmods[name].weight)
    ids = torch.randint(0, model.cfg.vocab_size, (2, 9),
                        generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        got, want = model(ids), ref(ids)
        # and the adapter is live: zeroing B changes the logits
        for m in ref.modules():
            if isinstance(m, LoRALinearModule):
                m.lora_B.zero_()
        no_adapter = ref(ids)
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-5), \
        (got - want).abs().max()
    assert (want - no_adapter).abs().max() > 1e-3


def test_quantize_model_defaults_and_errors():
    model = _tiny_lora_model()
    n = quantize_model_(model, 8)                # trainer call: unchanged
    assert n > 0
    assert any(isinstance(m, LoRALinearModule) for m in model.modules())
    assert not any(isinstance(m, QuantLoRALinear) for m in model.modules())
    with pytest.raises(ValueError):
        quantize_model_(nn.Sequential(nn.Linear(4, 4)), 8)   # nothing to do
    with pytest.raises(ValueError):
        quantize_model_(_tiny_lora_model(), 3)


# ------------------------------------------------------------------ serving
def test_build_model_quantized_generates():
    from datatunerx_amd.serve.engine import InferenceEngine, build_model
    cpu = torch.device("cpu")
    model = build_model("llama-tiny", cpu, quantization="int4")
    assert not any(isinstance(m, (FrozenLinear, LoRALinearModule))
                   for m in model.modules())
    assert all(m.bits == 4 for m in model.modules()
               if isinstance(m, QuantFrozenLinear))
    eng = InferenceEngine(model, device=cpu)
    out = eng.generate(list(range(4, 12)), max_new_tokens=4)
    assert out == eng.generate(list(range(4, 12)), max_new_tokens=4)
    assert len(out) <= 4
    assert isinstance(build_model("llama-tiny", cpu, quantization="int8"),
                      LlamaForCausalLM)
    with pytest.raises(ValueError, match="int3"):
        build_model("llama-tiny", cpu, quantization="int3")
    with pytest.raises(ValueError, match="llama"):
        build_model("gpt2-tiny", cpu, quantization="int8")


def test_server_quantization_flag(monkeypatch):
    from datatunerx_amd.serve import server
    args = server.parse_args(["--quantization", "int8", "--model",
                              "llama-tiny", "--port", "1"])
    assert args.quantization == "int8"
    assert server.parse_args([]).quantization is None
    with pytest.raises(SystemExit):
        server.parse_args(["--quantization", "fp8"])
    # main() hands the flag to build_model
    seen = {}

    class _Stop(Exception):
        pass

    def fake_build(name, device, adapter_dir=None, quantization=None):
        seen.update(name=name, quantization=quantization)
        raise _Stop

    import datatunerx_amd.serve.engine as engine
    monkeypatch.setattr(engine, "build_model", fake_build)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(_Stop):
        server.main(["--quantization", "int8", "--model", "llama-tiny"])
    assert seen == {"name": "llama-tiny", "quantization": "int8"}
    # refused at start-up: GPT-2, and tensor-parallel serving
    with pytest.raises(SystemExit, match="llama"):
        server.main(["--quantization", "int8", "--model", "gpt2-tiny"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="tensor-parallel"):
        server.main(["--quantization", "int4", "--model", "llama-tiny"])


# ------------------------------------------------------------ control plane
def _job(name, serve_cfg):
    from datatunerx_amd.api.types import FinetuneJob
    return FinetuneJob(name=name, spec={
        "fineTune": {"finetuneSpec": {
            "llm": "llama-tiny", "dataset": "ds",
            "hyperparameter": {"hyperparameterRef": "hp"}, "node": 1}},
        "serveConfig": serve_cfg})


def test_validation_serve_quantization():
    from datatunerx_amd.api.validation import ValidationError, validate_
    validate_(_job("q4", {"quantization": "int4"}))
    validate_(_job("q8", {"quantization": "int8", "tensorParallel": 1}))
    validate_(_job("none", {}))
    with pytest.raises(ValidationError, match="quantization"):
        validate_(_job("bad", {"quantization": "fp8"}))
    with pytest.raises(ValidationError, match="quantization"):
        validate_(_job("bad2", {"quantization": 4}))
    with pytest.raises(ValidationError, match="tensorParallel"):
        validate_(_job("tp", {"quantization": "int4", "tensorParallel": 2}))


class _FakeSupervisor:
    def __init__(self):
        self.calls = []

    def spawn(self, args, env, log, cwd):
        self.calls.append(list(args))
        return 4242


@pytest.mark.parametrize("quant", ["int4", None])
def test_reconcile_serve_passes_quantization(tmp_path, quant):
    from datatunerx_amd.api.controllers import (FinetuneJobController,
                                                ManagerConfig, PortAllocator)
    from datatunerx_amd.api.store import Store
    from datatunerx_amd.api.types import FinetuneJob
    store = Store(str(tmp_path / "state"))
    cfg = ManagerConfig(state_dir=str(tmp_path / "state"),
                        work_dir=str(tmp_path / "work"), cpu_mode=True)
    sup = _FakeSupervisor()
    ctl = FinetuneJobController(store, None, sup, cfg, PortAllocator(34500))
    job = _job("qserve", {"quantization": quant} if quant else {})
    job.status["state"] = "Serve"
    store.create(job)
    ctl._reconcile_serve(job)
    assert len(sup.calls) == 1
    argv = sup.calls[0]
    assert "datatunerx_amd.serve.server" in argv
    if quant:
        i = argv.index("--quantization")
        assert argv[i + 1] == quant
    else:
        assert "--quantization" not in argv
    cur = store.get(FinetuneJob, "default", "qserve")
    assert cur.status["serveInfo"]["pid"] == 4242
